"""Seeded scenarios for the hybrid re-rank with BOTH branches (graph nodes and vector hits) -- plain dictionaries in the shape of
tests/ranking_cases.py:scenario, fed to the REFERENCE's HybridRanker by tests/golden/gen_hybrid_goldens.py (expected rows in
tests/golden/ranking_hybrid_reference.json), to the host restatement by tests/test_hybrid_host.py and to crh_rerank_hybrid by
tests/test_rerank_hybrid_gpu.py.  Only inputs are made here.

Against ranking_cases.scenario: vector scores are multiples of 2^-12 (exact in f32, so the device starts from the numbers the
reference saw and every f64 result compares to the last bit); depths are 1..7 (the 0.3 floor of graph_match is reached at 5);
every name is <= 64 bytes and every query entity <= 48 bytes, so the device declines NO scenario; the centrality table holds
keys of primary entities and named hits only -- what QueryEngine._get_centrality_scores can have looked up (engine.py:348-377).
Small pools of names / files / lines make graph nodes meet vector hits on the merge key, two graph nodes meet each other,
files pass the per-file cap and totals pass 50; every fourth scenario plants a graph node and a hit whose scores tie exactly."""
import random

from tests.ranking_cases import FILES, INTENTS

NAMES = ["UserRepository", "verify_password", "login", "refresh", "hash_password", "BaseRepository", "CachedUserRepository", "parse",
         "parse_config", "Config", "config", "load", "Loader", "retry", "retry_with_backoff", "main", "", "Ünïcode", "x",
         "UserRepository.save", "Parser.parse_file", "a_very_long_entity_name_that_is_still_below_the_sixty_four_bytes", "löwe_ß", "do"]
ENTITIES = [n for n in NAMES if n and len(n.encode()) <= 48] + ["USERREPOSITORY", "pars", "Parse", "zzz", "", "LÖWE_ß"]
ROLES = ("primary_entities", "callers", "callees", "methods", "parent_classes", "child_classes")     # the ranker's order
LINES = [1, 1, 10, 20, 30]
N_HYBRID, HSEED = 64, 20261020
MAX_CANDIDATES = 512
assert all(len(n.lower().encode()) <= 64 for n in NAMES) and all(len(e.lower().encode()) <= 48 for e in ENTITIES)

# (intent, role, depth, summary?, docstring?, signature?, hit score * 4096, hit content length): a graph node of that role and a
# hit with that score whose final scores are EQUAL in f64 when neither matches an entity nor has a centrality entry -- found by
# enumerating the two formulas (scorer.py:68-74, :119-124), not by running the code under test
TIES = [("find_implementations", "callers", 2, True, False, False, 4096, 60), ("find_implementations", "callees", 3, False, True, False, 3072, 60),
        ("locate_entity", "callers", 5, False, False, False, 2560, 60), ("locate_entity", "callees", 6, True, True, True, 3328, 10),
        ("explain_data_flow", "callers", 4, False, False, True, 4096, 60), ("find_usages", "callers", 7, False, True, False, 4096, 60)]


def _where(rng, files, hot):
    """(name, file, line): four draws in ten come from the scenario's few HOT places, where merge keys meet."""
    if rng.random() < 0.4:
        return rng.choice(hot)
    return rng.choice(NAMES), rng.choice(files), rng.choice(LINES)


def _node(rng, depth_ok, files, hot):
    name, file, line = _where(rng, files, hot)
    meta = {"depth": rng.randrange(1, 8)} if depth_ok and rng.random() < 0.85 else {}
    return dict(node_type=rng.choice(["function", "class", "method"]), name=name, qualified_name=rng.choice([name, "app." + name]),
                file_path=file, start_line=line, end_line=line + rng.randrange(0, 40),
                signature=rng.choice([None, f"def {name}()"]), docstring=rng.choice([None, "Doc."]), summary=rng.choice([None, "Sums it up"]),
                metadata=meta)


def _hit(rng, score, files, hot):
    name, file, line = _where(rng, files, hot)
    n = rng.choice([0, 10, 50, 51, 60, 100, 101, 150, 1999, 2000, 2500, 2999, 3000, 4000])
    gid = rng.choice([None, name, "app." + name]) if name else None     # an unnamed hit is never looked up (engine.py:358-360)
    return dict(score=score, file_path=file, entity_type=rng.choice(["function", "class", "method", "file"]), entity_name=name,
                language=rng.choice(["python", "typescript"]), content=("x" * n) if n else rng.choice([None, ""]), start_line=line,
                end_line=line + 5, graph_node_id=gid, summary=rng.choice([None, "S"]))


def node_key(d):
    """The centrality key of a graph node dict or a hit dict (scorer.py:48-54)."""
    if "name" in d:
        return d["qualified_name"] or d["name"]
    return d.get("graph_node_id") or d.get("entity_name", "") or ""


def scenario(i):
    rng = random.Random(HSEED * 1000 + i)
    files = FILES if rng.random() < 0.6 else FILES + [f"pkg/m{j}.py" for j in range(17)]      # 7 files x 5 = 35 < 50 < 24 x 5
    hot = [(rng.choice(NAMES), rng.choice(files), rng.choice(LINES)) for _ in range(5)]
    graph = {role: [_node(rng, role in ("callers", "callees"), files, hot) for _ in range(rng.choice([0, 0, 1, 2, 4, 9]))] for role in ROLES}
    n_hits = rng.choice([0, 1, 3, 8, 20, 35, 70, 128])
    scores = sorted((rng.choice([0.5, 0.75, rng.randrange(-800, 4097) / 4096.0]) for _ in range(n_hits)), reverse=True)
    vector = [_hit(rng, s, files, hot) for s in scores]
    intent = rng.choice(INTENTS)
    entities = rng.sample(ENTITIES, rng.randrange(0, 5))
    if i % 4 == 0:
        # the planted tie: names outside the pools, so neither entry meets an entity (none are asked), a key or the table
        intent, role, depth, summ, doc, sig, num, clen = TIES[(i // 4) % len(TIES)]
        entities = []
        graph[role].append(dict(node_type="function", name=f"tie_node_{i}", qualified_name=f"tie.tie_node_{i}", file_path=f"tie/g{i}.py",
                                start_line=3, end_line=9, signature="def t()" if sig else None, docstring="Doc." if doc else None,
                                summary="Sums it up" if summ else None, metadata={"depth": depth}))
        vector.append(dict(score=num / 4096.0, file_path=f"tie/v{i}.py", entity_type="function", entity_name=f"tie_hit_{i}", language="python",
                           content="x" * clen, start_line=4, end_line=9, graph_node_id=None, summary=None))
        vector.sort(key=lambda h: -h["score"])
    keys = list(dict.fromkeys([node_key(n) for n in graph["primary_entities"]] + [node_key(h) for h in vector if h["entity_name"]]))
    keys = [k for k in keys if not k.startswith("tie")]
    cent = {k: {"in_degree": (d := rng.randrange(0, 80)), "out_degree": (o := rng.randrange(0, 80)), "total_degree": d + o, "relationship_count": d + o}
            for k in rng.sample(keys, min(len(keys), rng.randrange(0, 9)))}
    sc = dict(name=f"hybrid_{i}", intent=intent, entities=entities, graph=graph, vector=vector, centrality=rng.choice([cent, cent, cent, None]))
    assert sum(len(v) for v in graph.values()) + len(vector) <= MAX_CANDIDATES
    return sc


def scenarios():
    return [scenario(i) for i in range(N_HYBRID)]


def candidates(sc):
    """The concatenated candidate list as the ranker walks it: ``(role or None for a hit, dict)``, graph entries first."""
    return [(role, n) for role in ROLES for n in sc["graph"].get(role, [])] + [(None, h) for h in sc["vector"]]


def merge_key(d):
    return f"{d['file_path']}:{d['name'] if 'name' in d else d['entity_name']}:{d['start_line']}"


def depth_of(node):
    """``depth_from_query`` as ranker.py:96-99 reads it off a caller / callee node."""
    return node["metadata"].get("depth", 1) if node["metadata"] else 1
