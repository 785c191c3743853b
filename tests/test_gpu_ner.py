"""The ner model (non-equivalenced regions, src/model/ner.c) on the MI355X: the FAM_NER instantiations of the Viterbi kernels
(kernels/k_ner_*.hip, kmw_ner_*.hip) through the engine's public calls, against records of the reference itself
(tests/golden/ner_*_open0*.jsonl), against the lines the reference binary printed (tests/golden/ner_cli_*.json) and, for seeded
jobs that have no record, against the CPU oracle (pinned to the same records in tests/test_ner_model.py).  Integer work and
text: every comparison is exact."""
import random
import re

import pytest

import exonerate_amd as ex
from exonerate_amd import _abi
import oracle_lib
from golden_util import expected
from ner_cases import REFDUMP_SETS, SUBOPT_SETS, CLI_SETS, SUBOPT_MAX, open0_model, load_set, load_cli, cli_lines

pytestmark = pytest.mark.gpu


def _kernels(err):
    """names of the kernels a traced call launched (C4GPU_TRACE: `c4gpu trace:   kernel <name>: <n> workgroups per CU`)"""
    return re.findall(r"c4gpu trace:   kernel (k\w+):", err)


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(REFDUMP_SETS))
def test_find_score_and_path_match_reference_vectors(eng, name):
    model = open0_model(name)
    recs = load_set(name)
    pairs = [(r["query"], r["target"]) for r in recs]
    assert eng.find_score(model, pairs) == [r["score"] for r in recs]
    alns = eng.find_path(model, pairs, dpmemory=recs[0]["dpmemory"])
    for rec, aln in zip(recs, alns):
        assert aln is not None and aln.as_dict(rec["id"]) == expected(rec), rec["id"]


@pytest.mark.parametrize("name", sorted(REFDUMP_SETS))
def test_resident_batch_matches_reference_vectors(eng, name):
    model = open0_model(name)
    recs = load_set(name)
    b = ex.ResidentBatch(eng, model, [(r["query"], r["target"]) for r in recs])
    b.run(0)
    assert b.scores()[0] == [r["score"] for r in recs]
    b.run(2, dpmemory=recs[0]["dpmemory"])
    for i, rec in enumerate(recs):
        assert b.alignment(i).as_dict(rec["id"]) == expected(rec), rec["id"]
    b.close()


@pytest.mark.parametrize("name", sorted(SUBOPT_SETS))
def test_suboptimal_loop_matches_reference_vectors(eng, name):
    """GAM_Result_exhaustive_create's loop with SubOpt blocking (the `_sub` kernels): per-call rounds and the resident
    batch's next_paths, both against the successive alignments the reference produced."""
    model = open0_model(name)
    recs = load_set(name)
    pairs = [(r["query"], r["target"]) for r in recs]
    dpm, thr = recs[0]["dpmemory"], recs[0]["threshold"]
    found = eng.find_all_paths(model, pairs, dpmemory=dpm, threshold=thr, max_paths=SUBOPT_MAX)
    for rec, alns in zip(recs, found):
        assert len(alns) == len(rec["subopt"]), rec["id"]
        for a, exp in zip(alns, rec["subopt"]):
            assert (a.score, list(a.region), [list(o) for o in a.ops], a.vulgar(rec["id"])) == \
                   (exp["path_score"], exp["region"], exp["ops"], exp["vulgar"]), rec["id"]
    b = ex.ResidentBatch(eng, model, pairs)
    b.run(2, dpm, thr)
    rounds = [[b.alignment(i) for i in range(len(recs))]]
    while len(rounds) < SUBOPT_MAX and b.next_paths(dpm, thr) > 0:
        rounds.append([b.alignment(i) for i in range(len(recs))])
    b.close()
    for i, rec in enumerate(recs):
        got = [r[i] for r in rounds if r[i] is not None]
        assert [(a.score, list(a.region), [list(o) for o in a.ops], a.vulgar(rec["id"])) for a in got] == \
               [(e["path_score"], e["region"], e["ops"], e["vulgar"]) for e in rec["subopt"]], rec["id"]


@pytest.mark.parametrize("dpm", [32, 0])
@pytest.mark.parametrize("name", CLI_SETS)
def test_cli_sets_match_the_oracle_and_the_recorded_lines(eng, name, dpm, monkeypatch, capfd):
    """Other penalties than refdump's 0 (the default -20, -35), protein, and the two sets whose parameters switch the
    local-scope shortcut off by their magnitude (hugegap, hugeopen: Engine::local_exact): device alignments equal to the
    oracle's, and printed as the reference binary printed them."""
    data, model = load_cli(name)
    pairs = [(p["query"], p["target"]) for p in data["pairs"]]
    monkeypatch.setenv("C4GPU_TRACE", "1")
    scores = eng.find_score(model, pairs)
    alns = eng.find_path(model, pairs, dpmemory=dpm)
    err = capfd.readouterr().err
    launched = _kernels(err)
    assert launched and all("_ner_" in l for l in launched), launched
    if name in ("ner_cli_hugegap", "ner_cli_hugeopen"):
        assert not any("_local" in l for l in launched), launched          # every validity mask kept
    for pair, s, a in zip(data["pairs"], scores, alns):
        q, t = pair["query"].encode(), pair["target"].encode()
        assert s == oracle_lib.find_score(model.c, model.params, q, t), pair["id"]
        assert a.as_dict() == oracle_lib.find_path(model.c, model.params, q, t, dpmemory=dpm), pair["id"]
        assert cli_lines(data, pair, a) == pair["stdout"], pair["id"]


def test_local_shortcut_off_gives_the_same_batch(eng, monkeypatch, capfd):
    """C4GPU_LOCAL_EXACT=0 (the existing test hook) sends the score / region passes to the kernels that keep every validity
    mask: same scores, same alignments."""
    model = ex.Model("ner")
    recs = load_set("ner_dna_open0")
    pairs = [(r["query"], r["target"]) for r in recs]
    monkeypatch.setenv("C4GPU_TRACE", "1")

    def run():
        b = ex.ResidentBatch(eng, model, pairs)
        b.run(0)
        scores = b.scores()[0]
        b.run(2, dpmemory=0)
        out = [b.alignment(i).as_dict() for i in range(len(pairs))]
        b.close()
        return scores, out, _kernels(capfd.readouterr().err)
    on = run()
    monkeypatch.setenv("C4GPU_LOCAL_EXACT", "0")
    off = run()
    # (the continuation kernels' own mask-free form answers to another guard, Engine::cont_free_ok: not meant here)
    whole = [[k for k in names if "_cont" not in k] for names in (on[2], off[2])]
    assert whole[0] and all("_local" in k for k in whole[0]) and whole[1] and not any("_local" in k for k in whole[1]), whole
    assert on[:2] == off[:2]
    q, t = pairs[0]
    assert on[1][0] == oracle_lib.find_path(model.c, model.params, q.encode(), t.encode(), dpmemory=0)


def _rand(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def _sub(rng, s, rate, alpha="ACGT"):
    return "".join(rng.choice(alpha) if rng.random() < rate else c for c in s)


def _ner_pair(rng, qlen, tlen, alpha="ACGT"):
    """Three conserved blocks with unrelated inserts of different lengths between them, inside a target of tlen residues."""
    b = [_rand(rng, qlen // 3 - 20, alpha) for _ in range(3)]
    q = _rand(rng, 10, alpha) + b[0] + _rand(rng, 25, alpha) + b[1] + _rand(rng, 8, alpha) + b[2] + _rand(rng, 15, alpha)
    core = _sub(rng, b[0], 0.05, alpha) + _rand(rng, 9, alpha) + _sub(rng, b[1], 0.08, alpha) + _rand(rng, 47, alpha) + _sub(rng, b[2], 0.04, alpha)
    lead = max(0, tlen - len(core)) // 3
    return q, _rand(rng, lead, alpha) + core + _rand(rng, max(0, tlen - len(core) - lead), alpha)


def test_raw_viterbi_modes_match_oracle(eng):
    """Viterbi_DP_Func level, the four modes: score and region over the rectangle, a quadratic-space path, and checkpoint /
    path passes as continuation jobs (CORNER scopes, viterbi.c:68-76), DNA and protein."""
    import ctypes as C
    olib = oracle_lib.load()
    for alpha, a in (("ACGT", 0), ("ARNDCQEGHILKMFPSTWYV", 1)):
        model = ex.Model("ner", query_alphabet=a, target_alphabet=a, ner_open=-9)
        rng = random.Random(17 + a)
        q, t = _ner_pair(rng, 330, 520, alpha)
        region = (0, 0, len(q), len(t))

        def oracle(mode, reg, cont=None, cps=0):
            vo = oracle_lib.ViterbiOut()
            olib.oracle_viterbi(model.c, model.params, mode, q.encode(), len(q), t.encode(), len(t), _abi.Region(*reg), cont, cps, vo)
            out = {"score": vo.score, "query_start": vo.query_start, "target_start": vo.target_start, "query_end": vo.query_end,
                   "target_end": vo.target_end, "final_cell": list(vo.final_cell)[:vo.cell_size], "last_srp": vo.last_srp,
                   "ops": [vo.ops[k] for k in range(vo.n_ops)]}
            olib.oracle_viterbi_out_clear(vo)
            return out
        keys = ("score", "query_start", "target_start", "query_end", "target_end")
        got = eng.viterbi(model, ex.MODE_FIND_SCORE, [(q, t)], [{"pair": 0, "region": region}])[0]
        assert got["score"] == oracle(ex.MODE_FIND_SCORE, region)["score"]
        got = eng.viterbi(model, ex.MODE_FIND_REGION, [(q, t)], [{"pair": 0, "region": region}])[0]
        exp = oracle(ex.MODE_FIND_REGION, region)
        assert [got[k] for k in keys] == [exp[k] for k in keys]
        ar = (got["query_start"], got["target_start"], got["query_end"] - got["query_start"], got["target_end"] - got["target_start"])
        assert ar[2] > 200 and ar[3] > 200
        got = eng.viterbi(model, ex.MODE_FIND_PATH, [(q, t)], [{"pair": 0, "region": ar}])[0]
        exp = oracle(ex.MODE_FIND_PATH, ar)
        assert got["score"] == exp["score"] and got["ops"] == exp["ops"]
        assert any(model.c.transitions[o].label == _abi.LABEL_NER for o in got["ops"])
        # continuation jobs over the aligned region: START -> END, and between two inner states
        for first, final in ((model.c.start_state, model.c.end_state), (2, 2), (2, 5), (5, 2)):
            cont = _abi.Continuation()
            cont.first_state, cont.final_state = first, final
            cd = {"first_state": first, "final_state": final}
            sub = ar if first == model.c.start_state else (ar[0] + 7, ar[1] + 5, ar[2] - 40, ar[3] - 31)
            got = eng.viterbi(model, ex.MODE_FIND_CHECKPOINTS, [(q, t)], [{"pair": 0, "region": sub, "checkpoints": 4, "continuation": cd}])[0]
            exp = oracle(ex.MODE_FIND_CHECKPOINTS, sub, cont, 4)
            assert (got["score"], got["last_srp"], got["final_cell"][0]) == (exp["score"], exp["last_srp"], exp["final_cell"][0]), (first, final)
            got = eng.viterbi(model, ex.MODE_FIND_PATH, [(q, t)], [{"pair": 0, "region": sub, "continuation": cd}])[0]
            exp = oracle(ex.MODE_FIND_PATH, sub, cont)
            assert (got["score"], got["ops"]) == (exp["score"], exp["ops"]), (first, final)


def test_long_queries_run_the_multi_wave_kernels(eng, monkeypatch, capfd):
    """Queries of three and more 256-row strips (64 lanes x 4 rows: the engine takes the cooperating-wave form when a launch has
    at least three strips per job, c4_engine_launch.inc) against targets of a few thousand residues: kmw_ner_score_local and
    kmw_ner_region_local_pack must have run (the trace names every kernel launched), and the results are the oracle's."""
    model = ex.Model("ner")
    rng = random.Random(4)
    pairs = [_ner_pair(rng, ql, tl) for ql, tl in ((780, 2600), (1300, 2200))]
    monkeypatch.setenv("C4GPU_TRACE", "1")
    scores = eng.find_score(model, pairs)
    alns = eng.find_path(model, pairs, dpmemory=32)
    names = _kernels(capfd.readouterr().err)
    assert "kmw_ner_score_local" in names and "kmw_ner_region_local_pack" in names, names
    for (q, t), s, a in zip(pairs, scores, alns):
        assert s == oracle_lib.find_score(model.c, model.params, q.encode(), t.encode())
        assert a.as_dict() == oracle_lib.find_path(model.c, model.params, q.encode(), t.encode(), dpmemory=32)
        assert any(model.c.transitions[o[0]].label == _abi.LABEL_NER for o in a.ops)


def test_long_targets_take_the_windowed_region_pass(monkeypatch, capfd):
    """Targets long enough for the two-pass region scheme (a score pass that dumps columns, region windows started from a
    dump: kmw_ner_score_local_seed1 / kmw_ner_region_local_pack_seed2) give the oracle's alignments.  A context of its own:
    the engine leaves the scheme when the earlier batches of a context made it not pay."""
    model = ex.Model("ner")
    rng = random.Random(9)
    pairs = [_ner_pair(rng, 640, 33000)]
    monkeypatch.setenv("C4GPU_TRACE", "1")
    own = ex.Engine(0)
    try:
        alns = own.find_path(model, pairs, dpmemory=32)
    finally:
        own.close()
    err = capfd.readouterr().err
    assert "kmw_ner_score_local_seed1" in err and "kmw_ner_region_local_pack_seed2" in err, \
        [l for l in err.splitlines() if "kernel" in l]
    for (q, t), a in zip(pairs, alns):
        assert a.as_dict() == oracle_lib.find_path(model.c, model.params, q.encode(), t.encode(), dpmemory=32)


def test_device_sdp_refuses_ner(eng):
    """The device SDP has no ner passes (the ner state is a span along the query too): c4gpu_sdp_batch ends in an error, never
    in another family's kernels."""
    model = ex.Model("ner")
    q, t = _ner_pair(random.Random(2), 300, 500)
    with pytest.raises(ex.C4GpuError, match="no device passes"):
        eng.sdp(model, [(q, t)], [[[20, 60, 12, 60, 20]]])
