"""What does a literal text match (crh_text_match) cost -- against the arena's bytes, and against the host walk it
replaces (``store._RawClient._host_select``: ``str(value) in have`` over every alive payload)?  (profiles/text.md.)

    python tools/text_ab.py [--rows 100000,1000000] [--out FILE.json]

Arena: the bench's length mix -- tokens ~ clip(round(exp(N(ln 160, 0.8^2))), 8, 512) per chunk, as bench.py's embed leg -- at 4
bytes of text per token, drawn uniformly from a 47-entry table (letters, digits, blanks and newlines twice, the punctuation `_=().<>`).  One chunk
in 1000 holds `retry_after=`.  Uniform text has almost no false 4-byte prefixes (about 45^-4 per position); real code repeats its
prefixes more, and every false prefix costs a pass of the survivor loop -- the figures here are the streaming rate, not a promise
for a pattern like `self`.

Legs, each timed between device events on one stream after a warm-up (median, p10, p90 of --steps launches; no count is copied
back inside the window):

  p1   one 12-byte pattern, every row                      p8   eight patterns (ANY), every row
  p1f  one pattern under a 1/64 filter                     p8f  eight patterns under a 1/64 filter
       (a contiguous 64th of the rows, as a project filter leaves them: the other tiles' text is not read)
  c1   one pattern with ASCII case folding

GB/s = the arena's bytes (text + 8 per row of offsets) over the leg's time -- for the filtered legs the bytes of the rows the
filter leaves.  Beside it the float4-copy rate of the machine (6.29 TB/s: DESIGN.md 3.3) as the reference a streaming
kernel is read against.

  host  the Python loop of _host_select over the same chunks as str (``isinstance(v, str) and pat in v``), host clock, once --
        without that walk's per-slot payload-table lookup, so a LOWER bound of what the raw client's MatchText costs today.

The tool fails if a leg's words differ from ``bytes.find`` on the first 20 000 rows.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SYMBOLS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789  \n\n_=().<>", np.uint8)
NEEDLE = b"retry_after="
EIGHT = [NEEDLE, b".unwrap()", b"#include <hip/", b"TODO(", b"expect(", b"panic!(", b"__syncthreads", b"hipMalloc("]   # ANY of them
COPY_TBPS = 6.29


def summary(ms):
    return {"ms_median": round(float(np.median(ms)), 4), "ms_p10": round(float(np.percentile(ms, 10)), 4),
            "ms_p90": round(float(np.percentile(ms, 90)), 4), "steps": len(ms)}


def arena_rows(n, seed=0):
    """(row_off int64 [n + 1], bytes uint8): the length mix above, the needle written into every 1000th row that can hold it."""
    rng = np.random.default_rng(seed)
    lengths = 4 * np.clip(np.round(np.exp(rng.normal(np.log(160.0), 0.8, n))), 8, 512).astype(np.int64)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    data = SYMBOLS[rng.integers(0, SYMBOLS.size, size=int(off[-1]), dtype=np.uint8)]
    for r in range(0, n, 1000):
        at = int(off[r]) + int(lengths[r]) // 2
        data[at:at + len(NEEDLE)] = np.frombuffer(NEEDLE, np.uint8)
    return off, data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the host walk")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import coderag_amd  # noqa: F401
    from coderag_amd import ffi
    from tests import text_cases as tc

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    result = {"copy_rate_TBps": COPY_TBPS, "device": ffi.device_info(0), "sizes": []}
    for n in [int(v) for v in a.rows.split(",")]:
        off, data = arena_rows(n)
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
        out = torch.empty((words,), dtype=torch.int32, device=dev)
        legs = {"p1": ([NEEDLE], False, False, None), "p8": (EIGHT, False, True, None), "p1f": ([NEEDLE], False, False, mask),
                "p8f": (EIGHT, False, True, mask), "c1": ([NEEDLE.upper()], True, False, None)}
        size = {"rows": n, "text_bytes": int(off[-1]), "arena_bytes": nbytes, "filtered_bytes": fbytes, "legs": {}}
        head = min(n, 20000)
        head_rows = [data[off[r]:off[r + 1]].tobytes() for r in range(head)]
        for name, (pats, fold, anyp, m) in legs.items():
            _, count = arena.match(pats, fold_case=fold, any_of=anyp, mask=m, out=out, stream=stream)          # (with the count: waits)
            got = tc.mask_from_words(out[: (head + 31) // 32].cpu().numpy().view(np.uint32), head)
            want = tc.match_rows(head_rows, pats, fold, anyp, None if m is None else keep[:head])
            if not np.array_equal(got, want):
                raise SystemExit(f"{name} at {n} rows: the words differ from bytes.find on the first {head} rows")
            for _ in range(a.warmup):
                arena.match(pats, fold_case=fold, any_of=anyp, mask=m, out=out, count=False, stream=stream)
            ms = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                arena.match(pats, fold_case=fold, any_of=anyp, mask=m, out=out, count=False, stream=stream)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            s = summary(ms)
            read = fbytes if m is not None else nbytes
            s.update(count=count, bytes=read, GBps=round(read / (s["ms_median"] * 1e-3) / 1e9, 1))
            s["share_of_copy_rate"] = round(s["GBps"] / (COPY_TBPS * 1e3), 3)
            size["legs"][name] = s
            print(f"{n:>8} rows  {name:<4} {s['ms_median']:9.4f} ms (p10 {s['ms_p10']:.4f}, p90 {s['ms_p90']:.4f})  {s['GBps']:8.1f} GB/s "
                  f"of {read / 1e6:.1f} MB  count {count}", flush=True)
        if not a.no_host:
            texts = [data[off[r]:off[r + 1]].tobytes().decode("ascii") for r in range(n)]
            pat = NEEDLE.decode()
            t0 = time.perf_counter()
            found = sum(1 for v in texts if isinstance(v, str) and pat in v)
            dt = time.perf_counter() - t0
            size["host_walk"] = {"ms": round(dt * 1e3, 2), "count": found}
            size["host_over_p1"] = round(dt * 1e3 / size["legs"]["p1"]["ms_median"], 1)
            print(f"{n:>8} rows  host {dt * 1e3:9.2f} ms  count {found}  = {size['host_over_p1']} x p1", flush=True)
            if found != size["legs"]["p1"]["count"]:
                raise SystemExit("the host walk and the device disagree about the count")
            del texts
        result["sizes"].append(size)
        arena.close()
        del data, off
    line = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
