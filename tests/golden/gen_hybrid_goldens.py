#!/usr/bin/env python3
"""tests/golden/ranking_hybrid_reference.json: the REFERENCE's HybridRanker (src/lattice/query/ranking/*, loaded by path
exactly as gen_goldens.py does) run on the seeded graph + vector scenarios of tests/hybrid_cases.py.  Survey-container-only
(needs /root/reference); writes DATA only -- per result: entity_name, file_path, start_line, source, final_score and the seven
signals (null = the result does not carry that signal) -- the quantities the device re-rank decides.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_hybrid_goldens.py
"""
import json
import sys
from pathlib import Path

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
import gen_goldens  # noqa: E402
from tests import hybrid_cases  # noqa: E402

SIGNALS = ("graph_match", "query_entity_match", "relationship_relevance", "centrality", "context_richness", "vector_similarity",
           "code_quality")


def main():
    R = gen_goldens.load_reference()
    cases = []
    for i in range(hybrid_cases.N_HYBRID):
        sc = hybrid_cases.scenario(i)
        exp = gen_goldens.run_ranking(R, sc)["ranked"]
        cases.append({"name": sc["name"], "n": len(exp),
                      "rows": [[r["entity_name"], r["file_path"], r["start_line"], str(getattr(r["source"], "value", r["source"])), r["final_score"]]
                               + [r["signal_scores"].get(s) for s in SIGNALS] for r in exp]})
    out = {"generator": "tests/golden/gen_hybrid_goldens.py + tests/hybrid_cases.py:scenario", "seed": hybrid_cases.HSEED,
           "reference": "src/lattice/query/ranking/{models,scorer,ranker}.py",
           "columns": ["entity_name", "file_path", "start_line", "source", "final_score", *SIGNALS], "cases": cases}
    (HERE / "ranking_hybrid_reference.json").write_text(json.dumps(out, sort_keys=True, separators=(",", ":")))
    srcs = sorted({row[3] for c in cases for row in c["rows"]})
    print(f"wrote {len(cases)} cases; sources seen: {srcs}; sizes: {sorted({c['n'] for c in cases})}")


if __name__ == "__main__":
    main()
