#!/usr/bin/env python3
"""Pin oracle/encoder.py against the installed HF RobertaModel on rows up to the position table's end (1024 tokens) and freeze
tests/golden/encoder_long.npz: 12-layer base geometry with HF-init statistics, rows of 1024, 1023, 777 and 520 tokens padded to
1024, interior pad tokens on either side of key 512 in one row.  Same recipe and same checks as gen_encoder_goldens.py (whose
hf_forward it uses); weights are not stored but regenerated from the seed.  Needs `transformers`; never imported by the tests.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_encoder_goldens import ROOT, enc, hf_forward  # noqa: E402


def main():
    torch.manual_seed(0)
    cfg, seed, lengths, init = enc.EncoderConfig(), 37, [1024, 1023, 777, 520], "hf"
    w = enc.random_weights(cfg, seed, init=init)
    ids = enc.synthetic_ids(cfg, lengths, seed + 1, pad_to=1024)
    ids[2, 509] = cfg.pad_token_id            # interior pads around the 512-key boundary: masked as keys and in the pool
    ids[2, 514] = cfg.pad_token_id
    hs, ht = hf_forward(cfg, w, ids)
    os_, ot = enc.forward(w, cfg, ids, return_tokens=True)
    m = ids != cfg.pad_token_id
    err_s = np.abs(hs - os_).max()
    err_t = np.abs((ht - ot)[m]).max()
    print(f"long: oracle vs HF  max|d sent|={err_s:.2e}  max|d tok(valid)|={err_t:.2e}  |sent|~{np.abs(hs).mean():.3f}")
    assert err_s < 2e-5 and err_t < 1e-4
    solo = enc.forward(w, cfg, ids[3:4, : lengths[3]])       # pad invariance: the row alone equals its padded-batch row
    assert np.abs(solo[0] - os_[3]).max() < 2e-5
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "encoder_long.npz"), seed=seed, ids=ids, sent=hs, init=init,
                        cfg=np.array([cfg.vocab_size, cfg.hidden_size, cfg.num_layers, cfg.num_heads, cfg.intermediate_size,
                                      cfg.max_position_embeddings, cfg.type_vocab_size, cfg.pad_token_id]),
                        eps=cfg.layer_norm_eps)


if __name__ == "__main__":
    main()
