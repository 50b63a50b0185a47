"""CPU tier for chunks of up to 1023 tokens (the reference's ``max_length < 1024``): the oracle against the long-row HF fixture,
where ``max_length`` is validated, the provider's ``extra["max_length"]``, and the length-bucketing plan on a mix that reaches
the position table's end."""
import os

import numpy as np
import pytest

import coderag_amd  # noqa: F401
from coderag_amd import encoder as drv
from coderag_amd import providers as P
from oracle import encoder as orc

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_oracle_matches_long_hf_fixture():
    z = np.load(os.path.join(GOLD, "encoder_long.npz"))
    c = [int(v) for v in z["cfg"]]
    cfg = orc.EncoderConfig(vocab_size=c[0], hidden_size=c[1], num_layers=c[2], num_heads=c[3], intermediate_size=c[4],
                            max_position_embeddings=c[5], type_vocab_size=c[6], pad_token_id=c[7], layer_norm_eps=float(z["eps"]))
    ids = z["ids"]
    assert ids.shape == (4, 1024) and cfg.max_position_embeddings == 1026
    assert [int(np.flatnonzero(r != cfg.pad_token_id)[-1]) + 1 for r in ids] == [1024, 1023, 777, 520]
    got = orc.forward(orc.random_weights(cfg, int(z["seed"]), init=str(z["init"])), cfg, ids)
    assert np.abs(got - z["sent"]).max() < 3e-5          # HF RobertaModel fp32 (eager attention) on the same weights


@pytest.mark.parametrize("bad", [0, 4, 1024, 2000, -1, 512.0, True, "600"])
def test_max_length_outside_the_reference_range_is_rejected(bad):
    tok = drv.HashTokenizer(1000)
    with pytest.raises(ValueError, match="max_length"):
        drv.check_max_length(bad)
    with pytest.raises(ValueError, match="max_length"):
        drv.wrap_encoder_only(tok, "def f(): pass", bad)
    with pytest.raises(ValueError, match="max_length"):
        P.HipUniXcoderProvider(P.ProviderConfig(provider="unixcoder-hip", model="stub"), max_length=bad)
    with pytest.raises(ValueError, match="max_length"):
        P.HipUniXcoderProvider(P.ProviderConfig(provider="unixcoder-hip", model="stub", extra={"max_length": bad}))


@pytest.mark.parametrize("good", [5, 513, 1023, np.int64(700)])
def test_max_length_inside_the_reference_range_is_accepted(good):
    tok = drv.HashTokenizer(1000)
    assert drv.check_max_length(good) == int(good)
    text = " ".join(f"tok{i}" for i in range(1500))
    ids = drv.wrap_encoder_only(tok, text, good)
    assert len(ids) == int(good) and ids[:3] == [tok.cls_id, tok.enc_only_id, tok.sep_id] and ids[-1] == tok.sep_id
    p = P.HipUniXcoderProvider(P.ProviderConfig(provider="unixcoder-hip", model="stub"), max_length=good)
    assert p.max_length == int(good)


def test_provider_reads_max_length_from_extra():
    cfg = P.ProviderConfig(provider="unixcoder-hip", model="stub", extra={"max_length": 1023})
    assert P.HipUniXcoderProvider(cfg).max_length == 1023
    assert P.HipUniXcoderProvider(cfg, max_length=700).max_length == 700        # the argument wins over extra
    assert P.HipUniXcoderProvider(P.ProviderConfig(provider="unixcoder-hip", model="stub")).max_length == 512   # the reference's default

    class Stub:
        def __init__(self):
            self.seen = []

        def embed_texts(self, texts, max_length=512, **kw):
            self.seen.append(max_length)
            return [[0.0] for _ in texts]
    p = P.HipUniXcoderProvider(cfg)
    p._model = Stub()
    p._embed_sync(["x"])
    p.embed_texts_sync(["y"])
    assert p._model.seen == [1023, 1023]


def test_plan_batches_on_a_mix_that_reaches_1024():
    rng = np.random.default_rng(3)
    lengths = np.clip(np.round(np.exp(rng.normal(np.log(400), 0.9, 5000))), 5, 1024).astype(int)
    lengths[:4] = [1024, 1023, 513, 512]
    for packed in (False, True):
        batches = drv.HipUniXcoder.plan_batches(None, lengths, 65536, max_rows=4096, packed=packed)
        seen = sorted(i for rows, _ in batches for i in rows)
        assert seen == list(range(len(lengths)))
        for rows, Lmax in batches:
            assert Lmax % 16 == 0 and Lmax <= 1024 and Lmax >= max(int(lengths[i]) for i in rows)
            if packed:
                assert sum(int(lengths[i]) for i in rows) <= 65536 or len(rows) == 1
            else:
                assert Lmax * len(rows) <= 65536 or len(rows) == 1
        assert max(L for _, L in batches) == 1024
