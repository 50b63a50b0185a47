"""What does a regular-expression match (crh_text_regex) cost -- against the literal grep over the same arena, and
against the host walk with ``re`` it replaces?  (profiles/regex.md.)

    python tools/regex_ab.py [--rows 100000,1000000] [--out FILE.json]

Arena: tools/text_ab.py's -- the bench's length mix at 4 bytes of text per token, uniform over 47 symbols without upper case.  One
chunk in 1000 holds ``def parse_retry(`` and another one in 1000 ``TimeoutError `` (the only upper case there is).

Legs, each timed between device events on one stream after a warm-up (median, p10, p90 of --steps launches; no count is copied
back inside the window).  A leg with the prefilter is the two launches the store issues: crh_text_match for the expression's
required literals, crh_text_regex under its words.

  lit    ``def \\w+_retry\\(`` with the literal prefilter          lit0   the same, prefilter off (every row is walked)
  nolit  ``[A-Z][a-z]+(?:Error|Exception)\\b``: no required     big    ``a.{5}b``: 131 states, the largest table of the tests
         literal (the alternation hides it), every row is walked
  ...f   each of them under a 1/64 filter (a contiguous 64th of the rows, as a project filter leaves them)
  grep   crh_text_match, one 12-byte pattern (tools/text_ab.py's p1), for the same run's literal rate

GB/s = the arena's bytes (text + 8 per row of offsets) over the leg's time -- for the filtered legs the bytes of the rows the
filter leaves.

  host   ``re.compile(pattern, re.MULTILINE).search`` over the same chunks as bytes, host clock, once per pattern.

The tool fails if a leg's words differ from ``re`` on the first 20 000 rows.
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from text_ab import NEEDLE, arena_rows, summary  # noqa: E402

PLANTS = ((0, b"def parse_retry("), (500, b"TimeoutError "))
# ("nolit" is not `[A-Z][a-z]+Error\b`: that one HAS the required literal `Error` and runs like "lit")
PATTERNS = {"lit": r"def \w+_retry\(", "nolit": r"[A-Z][a-z]+(?:Error|Exception)\b", "big": r"a.{5}b"}


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
    from coderag_amd import ffi, regex_dfa
    from tests import regex_cases as rc
    from tests import text_cases as tc

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    result = {"device": ffi.device_info(0), "sizes": []}
    dfas = {name: regex_dfa.compile_regex(p) for name, p in PATTERNS.items()}
    if not dfas["lit"].literals or dfas["nolit"].literals or dfas["big"].literals:
        raise SystemExit("the legs' patterns no longer have the required literals their names promise")
    result["dfas"] = {name: {"pattern": PATTERNS[name], "states": d.n_states, "classes": d.n_classes, "literals": [lit.decode() for lit in d.literals]}
                      for name, d in dfas.items()}
    for n in [int(v) for v in a.rows.split(",")]:
        off, data = arena_rows(n)
        for first, plant in PLANTS:
            for r in range(first, n, 1000):
                at = int(off[r]) + 4
                data[at:at + len(plant)] = np.frombuffer(plant, np.uint8)
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
        pre = torch.empty((words,), dtype=torch.int32, device=dev)
        size = {"rows": n, "text_bytes": int(off[-1]), "arena_bytes": nbytes, "filtered_bytes": fbytes, "legs": {}}
        head = min(n, 20000)
        head_rows = [data[off[r]:off[r + 1]].tobytes() for r in range(head)]

        def launch(name, prefilter, m, count):
            if name == "grep":
                return arena.match([NEEDLE], mask=m, out=out, count=count, stream=stream)[1]
            d = dfas[name]
            if prefilter and d.literals:
                m = arena.match(d.literals, mask=m, out=pre, count=False, stream=stream)[0]
            return arena.regex(d, mask=m, out=out, count=count, stream=stream)[1]

        legs = [("lit", "lit", True), ("lit0", "lit", False), ("nolit", "nolit", True), ("big", "big", True), ("grep", "grep", False)]
        for leg, name, prefilter in legs:
            for filtered in (False, True):
                m = mask if filtered else None
                count = launch(name, prefilter, m, True)                                    # (with the count: waits)
                if name != "grep":
                    got = tc.mask_from_words(out[: (head + 31) // 32].cpu().numpy().view(np.uint32), head)
                    want = rc.match_rows(head_rows, PATTERNS[name], True, keep[:head] if filtered else None)
                    if not np.array_equal(got, want):
                        raise SystemExit(f"{leg} at {n} rows: the words differ from re on the first {head} rows")
                for _ in range(a.warmup):
                    launch(name, prefilter, m, False)
                ms = []
                for _ in range(a.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    launch(name, prefilter, m, False)
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                s = summary(ms)
                read = fbytes if filtered else nbytes
                s.update(count=count, bytes=read, GBps=round(read / (s["ms_median"] * 1e-3) / 1e9, 1))
                size["legs"][leg + ("f" if filtered else "")] = s
                print(f"{n:>8} rows  {leg + ('f' if filtered else ''):<6} {s['ms_median']:9.4f} ms (p10 {s['ms_p10']:.4f}, p90 {s['ms_p90']:.4f})  "
                      f"{s['GBps']:8.1f} GB/s of {read / 1e6:.1f} MB  count {count}", flush=True)
        if not a.no_host:
            texts = [data[off[r]:off[r + 1]].tobytes() for r in range(n)]
            size["host_walk"] = {}
            for name, p in PATTERNS.items():
                rx = re.compile(p.encode(), re.MULTILINE)
                t0 = time.perf_counter()
                found = sum(1 for v in texts if rx.search(v) is not None)
                dt = time.perf_counter() - t0
                size["host_walk"][name] = {"ms": round(dt * 1e3, 2), "count": found, "over_device": round(dt * 1e3 / size["legs"][name]["ms_median"], 1)}
                print(f"{n:>8} rows  host {name:<6} {dt * 1e3:9.2f} ms  count {found}  = {size['host_walk'][name]['over_device']} x the device", flush=True)
                if found != size["legs"][name]["count"]:
                    raise SystemExit(f"the host walk and the device disagree about the count of {name}")
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
