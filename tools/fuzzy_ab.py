"""What does an approximate substring match (crh_text_fuzzy) cost -- with and without the pigeonhole prefilter,
under a filter, against the regex walk and the literal grep over the same arena, and against the host restatement it replaces?
(profiles/fuzzy.md.)

    python tools/fuzzy_ab.py [--rows 1000000] [--out FILE.json]

Arena: tools/text_ab.py's -- the bench's length mix at 4 bytes of text per token, uniform over 47 symbols without upper case.  For
every pattern one chunk in 1000 holds it exactly, another one in 1000 with one byte left out, a third with one byte left out
and another one replaced (where the chunk is long enough).

Patterns: 8, 32 and 64 bytes (the 32-bit state, its last length, the 64-bit state's last length), each with 1, 2 and 3 edits.
Legs, each timed between device events on one stream after a warm-up (median, p10, p90 of --steps launches; no count is copied
back inside the window):

  walk   crh_text_fuzzy over every row
  pre    the two launches the store issues when its rule cuts pieces (store.fuzzy_pieces: the shortest of the k + 1 pieces has at
         least 3 bytes): crh_text_match for ANY of the pieces, crh_text_fuzzy under its words; absent where the rule cuts none
  ...f   each of them under a 1/64 filter (a contiguous 64th of the rows, as a project filter leaves them)
  regex  crh_text_regex, ``[A-Z][a-z]+(?:Error|Exception)\\b`` (tools/regex_ab.py's "nolit": every row is walked)   } the same
  grep   crh_text_match, one 12-byte pattern (tools/text_ab.py's p1)                                              } run's rates

GB/s = the arena's bytes (text + 8 per row of offsets) over the leg's time -- for the filtered legs the bytes of the rows the
filter leaves.

  host   the restatement of tests/fuzzy_cases.py (Sellers' table in numpy) over the first --sample rows, host clock, scaled to
         the arena's rows.

The tool fails if any level's words differ from the restatement on the sample, or if a prefiltered leg's counts differ from
the plain walk's.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from text_ab import NEEDLE, arena_rows, summary  # noqa: E402

BASE = b"parse_retry_after_seconds(response.headers)_or_default_backoff=1"       # 64 bytes of the arena's own symbols
LENGTHS, EDITS = (8, 32, 64), (1, 2, 3)
REGEX = r"[A-Z][a-z]+(?:Error|Exception)\b"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=2000, help="rows the host restatement walks (and the device is checked on)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi, regex_dfa
    from coderag_amd.store import fuzzy_pieces
    from tests import fuzzy_cases as fc
    from tests import text_cases as tc

    assert len(BASE) == 64
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n = a.rows
    off, data = arena_rows(n)
    patterns = {m: BASE[:m] for m in LENGTHS}
    for j, m in enumerate(LENGTHS):
        p = patterns[m]
        forms = (p, fc.delete(p, m // 2), fc.substitute(fc.delete(p, m // 2), 2, ord("q")))
        for e, form in enumerate(forms):
            for r in range(10 * (3 * j + e) + 1, n, 1000):
                if off[r + 1] - off[r] >= len(form) + 8:
                    at = int(off[r]) + 4
                    data[at:at + len(form)] = np.frombuffer(form, np.uint8)
    arena = ffi.Text(capacity_rows=n, capacity_bytes=int(off[-1]), device=0)
    for r0 in range(0, n, 65536):
        r1 = min(n, r0 + 65536)
        arena.append(off[r0:r1 + 1] - off[r0], data[off[r0]:off[r1]])
    nbytes = int(off[-1]) + 8 * (n + 1)
    words = (n + 31) // 32
    lo, hi = (n // 3) // 32 * 32, (n // 3) // 32 * 32 + max(32, n // 64 // 32 * 32)      # the filter's rows: a contiguous 64th, whole tiles
    keep = np.zeros(n, bool)
    keep[lo:hi] = True
    mask = torch.from_numpy(tc.words_from_mask(keep).view(np.int32).copy()).to(dev)
    fbytes = int(off[hi] - off[lo]) + 8 * (hi - lo + 1)
    pre = torch.empty((words,), dtype=torch.int32, device=dev)
    one = torch.empty((words,), dtype=torch.int32, device=dev)
    head = min(n, a.sample)
    head_rows = [data[off[r]:off[r + 1]].tobytes() for r in range(head)]
    result = {"device": ffi.device_info(0), "rows": n, "text_bytes": int(off[-1]), "arena_bytes": nbytes, "filtered_bytes": fbytes,
              "sample": head, "legs": {}, "host": {}}

    def timed(launch):
        for _ in range(a.warmup):
            launch(False)
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(False)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return summary(ms)

    def report(leg, s, read, count):
        s.update(count=count, bytes=read, GBps=round(read / (s["ms_median"] * 1e-3) / 1e9, 1))
        result["legs"][leg] = s
        print(f"{leg:<12} {s['ms_median']:9.4f} ms (p10 {s['ms_p10']:.4f}, p90 {s['ms_p90']:.4f})  {s['GBps']:8.1f} GB/s of {read / 1e6:.1f} MB  count {count}", flush=True)

    for m in LENGTHS:
        p = patterns[m]
        t0 = time.perf_counter()
        dist = fc.distances(head_rows, p)
        host_ms = (time.perf_counter() - t0) * 1e3
        result["host"][f"m{m}"] = {"sample_ms": round(host_ms, 2), "scaled_to_rows_ms": round(host_ms * n / head, 1)}
        print(f"host m{m}: {host_ms:.1f} ms for {head} rows = {host_ms * n / head / 1e3:.1f} s for {n}", flush=True)
        for k in EDITS:
            pieces = fuzzy_pieces(p, k)
            levels = torch.empty((k + 1, words), dtype=torch.int32, device=dev)
            plain = {}
            for prefilter in (False, True):
                if prefilter and not pieces:
                    continue
                for filtered in (False, True):
                    m0 = mask if filtered else None

                    def launch(count, m0=m0, prefilter=prefilter):
                        under = arena.match(pieces, any_of=True, mask=m0, out=pre, count=False, stream=stream)[0] if prefilter else m0
                        return arena.fuzzy(p, k, mask=under, out=levels, count=count, stream=stream)[1]

                    counts = launch(True)                                  # (with the counts: waits)
                    got = np.stack([tc.mask_from_words(w, head) for w in levels[:, : (head + 31) // 32].cpu().numpy().view(np.uint32)])
                    want = fc.levels(head_rows, p, k, mask=keep[:head] if filtered else None, dist=dist)
                    if not np.array_equal(got, want):
                        raise SystemExit(f"m{m} k{k}: the words differ from the restatement on the first {head} rows")
                    if prefilter and counts != plain[filtered]:
                        raise SystemExit(f"m{m} k{k}: the prefilter changes the counts: {counts} against {plain[filtered]}")
                    plain.setdefault(filtered, counts)
                    leg = f"m{m}k{k}_" + ("pre" if prefilter else "walk") + ("f" if filtered else "")
                    report(leg, timed(launch), fbytes if filtered else nbytes, counts)
                    if prefilter:
                        result["legs"][leg]["pieces"] = [x.decode() for x in pieces]

    dfa = regex_dfa.compile_regex(REGEX)
    for filtered in (False, True):
        m0 = mask if filtered else None
        count = arena.regex(dfa, mask=m0, out=one, stream=stream)[1]
        report("regex" + ("f" if filtered else ""), timed(lambda c, m0=m0: arena.regex(dfa, mask=m0, out=one, count=c, stream=stream)), fbytes if filtered else nbytes, count)
        count = arena.match([NEEDLE], mask=m0, out=one, stream=stream)[1]
        report("grep" + ("f" if filtered else ""), timed(lambda c, m0=m0: arena.match([NEEDLE], mask=m0, out=one, count=c, stream=stream)), fbytes if filtered else nbytes, count)
    arena.close()
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
