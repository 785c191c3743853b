"""The translated models -- ungapped:trans and coding2coding, the only families whose transitions advance the query by more than
one row (c4_viterbi_kernel.h, WaveDP::AQ = 3) -- on the MI355X against the CPU oracle, which restates their 3:3 match and is
pinned on the reference's records and on the reference run live at one to five strips (tests/test_oracle_codon.py).  With the
oracle these kernels are held at what no record reaches: queries whose last 256-row strip holds one to four rows, transitions of
every advance across a lane edge, a strip edge and the carry row in HBM, raw Viterbi modes and continuations, regions that start
at any row, a 33 000-column target, staged batches, and a fuzz over one to five strips.  Nothing here needs refdump.  Integer work
and text: every comparison is exact."""
import os
import random
import re

import pytest

import exonerate_amd as ex
from exonerate_amd import _abi
import oracle_lib
from codon_cases import (POINTS, EDGE_POINTS, BANDS, STRIP, AA, CODONS, edge_pairs, fuzz_pair, band_shows, band_rng,
                         point_model)

pytestmark = pytest.mark.gpu
FAMILY_TAG = {"coding2coding": "_coding2coding_", "ungapped:trans": "_ungapped_codon_"}
MODELS = sorted(FAMILY_TAG)


def _kernels(err):
    """names of the kernels a traced call launched (C4GPU_TRACE: `c4gpu trace:   kernel <name>: <n> workgroups per CU`)"""
    return re.findall(r"c4gpu trace:   kernel (k\w+):", err)


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


def _opath(model, q, t, dpm=32, thr=_abi.IMPOSSIBLY_LOW_SCORE):
    return oracle_lib.find_path(model.c, model.params, q.encode(), t.encode(), dpmemory=dpm, threshold=thr)


def _dicts(alns):
    return [a.as_dict() if a is not None else None for a in alns]


# ---- strip and lane edges -------------------------------------------------------------------------------------------------
_BAND = {}


def _band(model_type, k, point, what):
    """The band's pairs and the oracle's answer to `what` ("score", 32 or 0: find_path at that dpmemory), computed once."""
    key = (model_type, k, point)
    if key not in _BAND:
        _BAND[key] = {"model": point_model(model_type, point),
                      "pairs": edge_pairs(model_type, k, band_rng(model_type, k))}
    b = _BAND[key]
    if what not in b:
        m = b["model"]
        b[what] = [oracle_lib.find_score(m.c, m.params, q.encode(), t.encode()) if what == "score" else _opath(m, q, t, what)
                   for q, t in b["pairs"]]
    return b["model"], b["pairs"], b[what]


def _run_band(eng, capfd, model_type, k, point, dpm):
    """find_score (with the dpmemory 32 case) and find_path over the band's batch; returns the kernels find_path launched."""
    model, pairs, exp = _band(model_type, k, point, dpm)
    capfd.readouterr()
    if dpm == 32:
        assert eng.find_score(model, pairs) == _band(model_type, k, point, "score")[2]
        launched = _kernels(capfd.readouterr().err)
        assert launched and all(FAMILY_TAG[model_type] in n and "_score" in n for n in launched), launched
    got = _dicts(eng.find_path(model, pairs, dpmemory=dpm))
    launched = _kernels(capfd.readouterr().err)
    assert launched and all(FAMILY_TAG[model_type] in n for n in launched), launched
    for n, (g, e) in enumerate(zip(got, exp)):
        assert g == e, (model_type, k, point, dpm, n, len(pairs[n][0]), len(pairs[n][1]))
    return launched


# Parameter points of the sweep: the first of codon_cases.EDGE_POINTS for each model (coding2coding: cheap, where the path takes
# every event at the boundary; ungapped:trans: default).  The second (coding2coding: default; ungapped:trans: codonalt) was cut for
# the GPU suite's time; tests/test_oracle_codon.py still runs both on the CPU against the reference.
SWEEP_POINTS = [0]


@pytest.mark.parametrize("dpm", [32, 0])
@pytest.mark.parametrize("nth_point", SWEEP_POINTS)
@pytest.mark.parametrize("k", BANDS)
@pytest.mark.parametrize("model_type", MODELS)
def test_strip_and_lane_edges(eng, model_type, k, nth_point, dpm, monkeypatch, capfd):
    """codon_cases.edge_pairs: queries of 256 k - 2 ... 256 k + 3 bases (the last strip holds one to four rows, fewer than an
    advance) and of 1 ... 13 bases (fewer rows than an advance; lane edges at multiples of 4), in all three frames, one batch per
    band: the oracle's scores and alignments, with every kernel of the model's own family."""
    monkeypatch.setenv("C4GPU_TRACE", "1")
    launched = _run_band(eng, capfd, model_type, k, EDGE_POINTS[model_type][nth_point], dpm)
    if dpm == 0 and k != "small":         # (13 rows are at most 6 x the largest advance: Viterbi_use_reduced_space says no)
        assert any("_ckpt_cont" in n for n in launched) and any("_path_cont" in n for n in launched), launched


@pytest.mark.parametrize("k", BANDS[1:])
@pytest.mark.parametrize("model_type", MODELS)
def test_the_bands_cross_their_boundaries(model_type, k):
    """What makes the test above a test of the multi-row exchange, decided by the oracle's alignments alone: at every parameter
    point of the sweep an advance of 3 goes from a row below 256 k to a row at or above it, and over the points so does every advance the model
    has (ungapped:trans: landing 0, 1 and 2 rows past the boundary), in the query's rows -- the strips of the score and region
    passes -- and in rows counted from the alignment's start -- those of the path, checkpoint and continuation passes; and
    coding2coding takes each of its six events (a base, two bases, a codon, on either axis) at a row 256 k - 3 ... 256 k + 3
    (codon_cases.band_shows).  A band that does not show this fails."""
    missing = band_shows(model_type, k, {point: _band(model_type, k, point, 32)[2]
                                          for point in [EDGE_POINTS[model_type][n] for n in SWEEP_POINTS]})
    assert missing is None, (model_type, k, missing)


def test_edges_with_the_shortcuts_off(eng, monkeypatch, capfd):
    """C4GPU_LOCAL_EXACT=0, C4GPU_CONT_FREE=0 and C4GPU_PACK=0 send every pass to the kernels that keep the validity masks -- for
    an advance of a: i - a >= 0 -- and to the two-slot region start: the band of the first strip edge gives the same."""
    monkeypatch.setenv("C4GPU_TRACE", "1")
    on = _run_band(eng, capfd, "coding2coding", 1, "cheap", 32) + _run_band(eng, capfd, "coding2coding", 1, "cheap", 0)
    monkeypatch.setenv("C4GPU_LOCAL_EXACT", "0")
    monkeypatch.setenv("C4GPU_CONT_FREE", "0")
    monkeypatch.setenv("C4GPU_PACK", "0")
    off = _run_band(eng, capfd, "coding2coding", 1, "cheap", 32) + _run_band(eng, capfd, "coding2coding", 1, "cheap", 0)
    assert any("_local" in n for n in on) and not any("_local" in n or "_pack" in n for n in off), (on, off)


def test_edges_with_a_penalty_that_switches_the_local_shortcut_off(eng, monkeypatch, capfd):
    """--frameshift -350000000: Engine::local_exact is off by the parameters' magnitude, no test hook involved, so the general
    kernels with every per-transition mask serve the whole batch."""
    monkeypatch.setenv("C4GPU_TRACE", "1")
    launched = _run_band(eng, capfd, "coding2coding", 1, "huge", 32) + _run_band(eng, capfd, "coding2coding", 1, "huge", 0)
    assert not any("_local" in n for n in launched), launched
    assert any("_ckpt_cont" in n for n in launched), launched


# ---- raw Viterbi modes ----------------------------------------------------------------------------------------------------
def _coding_pair(rng, codons, lead, trail, events=True):
    """A homologous coding pair of `codons` codons with a one- and a two-base frameshift in the query, a two-base one in the
    target and a codon indel, the target inside
    `lead` + `trail` unrelated bases."""
    pep = [rng.choice(AA) for _ in range(codons)]
    qc = [rng.choice(CODONS[a]) for a in pep]
    tc = [rng.choice(CODONS[rng.choice(AA) if rng.random() < 0.1 else a]) for a in pep]
    if events:
        qc[codons // 4] += rng.choice("ACGT")
        qc[3 * codons // 8] += "".join(rng.choice("ACGT") for _ in range(2))
        tc[codons // 2] += "".join(rng.choice("ACGT") for _ in range(2))
        del tc[3 * codons // 4]
    dna = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    return dna(rng.randint(0, 2)) + "".join(qc) + dna(2), dna(lead) + "".join(tc) + dna(trail)


@pytest.mark.parametrize("model_type", MODELS)
def test_raw_viterbi_modes_match_oracle(eng, model_type):
    """Viterbi_DP_Func level, the four modes, on a query of two strips: score and region over the rectangle, a quadratic-space
    path, and checkpoint / path passes as continuation jobs (CORNER scopes, viterbi.c:68-76) from START to END and between inner
    states, over sub-regions that begin inside a strip at a query offset that is no multiple of 3: row 0 of such a job is its own
    first row, and an advance of a is valid from row a on."""
    olib = oracle_lib.load()
    coding = model_type == "coding2coding"
    model = point_model(model_type, "cheap" if coding else "default")
    rng = random.Random(23 + len(model_type))
    q, t = _coding_pair(rng, 110, 40, 70, events=coding)
    assert len(q) >= 300
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
    assert ar[2] > 290 and ar[3] > 290
    got = eng.viterbi(model, ex.MODE_FIND_PATH, [(q, t)], [{"pair": 0, "region": ar}])[0]
    exp = oracle(ex.MODE_FIND_PATH, ar)
    assert got["score"] == exp["score"] and got["ops"] == exp["ops"]
    advances = {model.c.transitions[o].advance_query for o in got["ops"]}
    assert advances >= ({1, 2, 3} if coding else {3}), advances
    start, end, match, fsq, fst = model.c.start_state, model.c.end_state, 2, 5, 6
    # (first state, final state, sub-region): the aligned region, then pieces of it that start at rows 7, 8 and 9 past its first
    # row (7 = 1, 8 = 2, 9 = 0 mod 3) and inside the first strip; ungapped:trans has one diagonal per job, so its pieces are square
    if coding:
        conts = [(start, end, ar), (match, match, (ar[0] + 7, ar[1] + 5, ar[2] - 40, ar[3] - 31)),
                 (match, fsq, (ar[0] + 8, ar[1] + 6, ar[2] - 40, ar[3] - 31)), (fsq, match, (ar[0] + 9, ar[1] + 4, ar[2] - 41, ar[3] - 33)),
                 (match, fst, (ar[0] + 7, ar[1] + 9, ar[2] - 38, ar[3] - 30)), (fst, match, (ar[0] + 8, ar[1] + 5, 271, 280))]
    else:
        conts = [(start, end, ar), (match, match, (ar[0] + 7, ar[1] + 7, ar[2] - 42, ar[3] - 42)),
                 (match, match, (ar[0] + 8, ar[1] + 5, 270, 270)), (match, end, (ar[0] + 9, ar[1] + 9, 258, 258))]
    for first, final, sub in conts:
        assert first == start or (sub[0] % STRIP not in (0, STRIP - 1) and sub[0] + sub[2] > STRIP), sub
        cont = _abi.Continuation()
        cont.first_state, cont.final_state = first, final
        cd = {"first_state": first, "final_state": final}
        got = eng.viterbi(model, ex.MODE_FIND_CHECKPOINTS, [(q, t)], [{"pair": 0, "region": sub, "checkpoints": 4, "continuation": cd}])[0]
        exp = oracle(ex.MODE_FIND_CHECKPOINTS, sub, cont, 4)
        assert (got["score"], got["last_srp"], got["final_cell"][0]) == (exp["score"], exp["last_srp"], exp["final_cell"][0]), (first, final, sub)
        got = eng.viterbi(model, ex.MODE_FIND_PATH, [(q, t)], [{"pair": 0, "region": sub, "continuation": cd}])[0]
        exp = oracle(ex.MODE_FIND_PATH, sub, cont)
        assert (got["score"], got["ops"]) == (exp["score"], exp["ops"]), (first, final, sub)


# ---- regions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dpm", [32, 0])
@pytest.mark.parametrize("model_type", MODELS)
def test_run_regions_match_oracle(eng, model_type, dpm):
    """ResidentBatch.run_regions (Optimal_find_path over a region, what --refine region asks for): regions whose first query row
    is 0, 1, 2 mod 3 and row 255, 256 and 257 of the query -- the region's first row is row 0 of the job, so the transitions of
    advance a are masked by i - a >= 0 in the job's own rows, wherever the region lies in the query -- with 1, 2 and 3 query rows
    and with two strips of them."""
    coding = model_type == "coding2coding"
    model = point_model(model_type, "cheap" if coding else "default")
    rng = random.Random(41 + len(model_type))
    q, t = _coding_pair(rng, 250, 30, 60, events=coding)
    Q, T = len(q), len(t)
    assert Q > 700
    regions = [(0, 0, Q, T), (1, 3, Q - 1, T - 3), (2, 0, Q - 2, T), (3, 7, 300, 340), (4, 20, 1, 30), (5, 20, 2, 30), (6, 20, 3, 30),
               (7, 20, 4, 33), (255, 270, 300, 330), (256, 270, 300, 330), (257, 270, 300, 330), (255, 280, 3, 40),
               (256, 280, 2, 40), (257, 280, 1, 40), (100, 120, 2 * STRIP + 2, T - 130), (Q - 2, T - 30, 2, 30)]
    assert {r[0] % 3 for r in regions} == {0, 1, 2} and {r[2] for r in regions} >= {1, 2, 3}
    assert all(r[0] + r[2] <= Q and r[1] + r[3] <= T for r in regions)
    b = ex.ResidentBatch(eng, model, [(q, t)] * len(regions))
    b.run_regions(regions, dpmemory=dpm)
    got = _dicts([b.alignment(i) for i in range(len(regions))])
    b.close()
    found = 0
    for reg, g in zip(regions, got):
        exp = oracle_lib.find_path_region(model.c, model.params, q.encode(), t.encode(), reg, dpmemory=dpm)
        assert g == exp, (model_type, dpm, reg)
        found += exp is not None and exp["score"] > 0
    assert found >= 8


# ---- long target ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_type", MODELS)
def test_long_target(model_type, monkeypatch, capfd):
    """About 300 x 33 000 with the homologous stretch beyond column 16 384, in a context of its own (as the ner test of the
    windowed region pass): these families have no seeded-window kernels, so none may run, and the alignment is the oracle's."""
    coding = model_type == "coding2coding"
    model = point_model(model_type, "default")
    rng = random.Random(57 + len(model_type))
    q, t = _coding_pair(rng, 100, 20000 + rng.randint(0, 2), 12800, events=coding)
    assert len(q) >= 300 and len(t) >= 33000
    monkeypatch.setenv("C4GPU_TRACE", "1")
    own = ex.Engine(0)
    try:
        score = own.find_score(model, [(q, t)])[0]
        aln = own.find_path(model, [(q, t)], dpmemory=32)[0]
    finally:
        own.close()
    err = capfd.readouterr().err
    launched = _kernels(err)
    assert launched and all(FAMILY_TAG[model_type] in n and "seed" not in n for n in launched), launched
    assert "seeded pass" not in err
    exp = _opath(model, q, t)
    assert score == exp["score"] and aln.as_dict() == exp
    assert exp["region"][1] > 16384 and exp["region"][2] > 250, exp["region"]


# ---- staged batches ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_type", MODELS)
def test_staged_batches_match_oracle(eng, model_type):
    """Stage.load + swap on a codon batch, two swaps in a row (ResidentSeqs::build, family_is_codon: every unique query is
    translated once): batches of different sizes and lengths, the second's queries shorter than the first's -- a translated code
    left over from the first batch would show -- and in both one query object shared by several pairs."""
    coding = model_type == "coding2coding"
    model = point_model(model_type, "default")
    rng = random.Random(71 + len(model_type))

    def batch(sizes, shared_codons, n_shared):
        pairs = [_coding_pair(rng, c, rng.randint(0, 40), rng.randint(0, 40), events=coding) for c in sizes]
        sq, st = _coding_pair(rng, shared_codons, 10, 10, events=False)
        sq = sq.encode()                                                   # one bytes object: one buffer for all of its pairs
        for n in range(n_shared):
            tt = "".join(rng.choice("ACGT") if rng.random() < 0.04 else c for c in st)
            pairs.insert(1 + 2 * n, (sq, tt[3 * n:]))
        return pairs
    first = batch([150, 95, 120, 180], 130, 3)
    second = batch([40, 9, 61], 52, 2)
    third = batch([70, 30, 100, 12, 55], 88, 4)
    assert max(len(q) for q, _ in second) < min(len(q) for q, _ in first)
    stage = ex.Stage(eng, model)
    stage.load(first)
    b = ex.ResidentBatch(eng, model, third[:2])                   # any batch: it is swapped out before the first run
    for k, pairs in enumerate((first, second, third)):
        b.swap(stage)
        if k == 0:
            stage.load(second)                                             # into the buffers the batch handed back
        elif k == 1:
            stage.load(third)
        b.run(0)
        scores = b.scores()[0]
        b.run(2)
        for i, (q, t) in enumerate(pairs):
            q = q.decode() if isinstance(q, bytes) else q
            exp = _opath(model, q, t)
            a = b.alignment(i)
            assert (a.as_dict() if a is not None else None) == exp, (model_type, k, i)
            assert scores[i] == oracle_lib.find_score(model.c, model.params, q.encode(), t.encode()), (model_type, k, i)
    b.close()
    stage.close()


# ---- library fuzz -----------------------------------------------------------------------------------------------------------
# C4_FUZZ_SEED / C4_FUZZ_REPS: longer one-off campaigns with other seeds.  Default: 4 committed seeds (6 at first; two were cut
# for the GPU suite's time), the base chosen so that the four draw both models with and without sub-optimal rounds, the three
# parameter points (cheap with coding2coding alone, which it concerns), dpmemory 0 / 1 / 32, all three thresholds, and queries of
# one, two, three and five strips
@pytest.mark.parametrize("seed", range(int(os.environ.get("C4_FUZZ_REPS", "2")) * 2))
def test_codon_library_fuzz(eng, seed):
    """Engine.find_path / find_all_paths against the oracle on seeded random batches of the two translated models: queries of
    one to five strips, three parameter points, dpmemory 0 / 1 / 32, thresholds, up to three sub-optimal rounds."""
    base = int(os.environ.get("C4_FUZZ_SEED", "10402"))
    rng = random.Random(base + seed)
    model_type = rng.choice(MODELS)
    point = rng.choice(sorted(POINTS))
    model = point_model(model_type, point)
    dpm = rng.choice([0, 1, 32])
    thr = rng.choice([-987654321, 50, 200])
    rounds = rng.choice([1, 1, 2, 3])
    pairs = [fuzz_pair(rng) for _ in range(rng.randint(1, 4))]
    what = "C4_FUZZ_SEED=%d seed %d: %s %s dpmemory %d threshold %d rounds %d" % (base, seed, model_type, point, dpm, thr, rounds)
    if rounds == 1:
        got = [[a] if a else [] for a in eng.find_path(model, pairs, dpmemory=dpm, threshold=thr)]
    else:
        got = eng.find_all_paths(model, pairs, dpmemory=dpm, threshold=max(thr, 40), max_paths=rounds)
    for n, ((q, t), alns) in enumerate(zip(pairs, got)):
        if rounds == 1:
            e = _opath(model, q, t, dpm, thr)
            exp = [e] if e else []
        else:
            exp = [d for d, _ in oracle_lib.find_paths_subopt(model.c, model.params, q.encode(), t.encode(), dpm, max(thr, 40), rounds)]
        assert [a.as_dict() for a in alns] == exp, "%s, pair %d (%d x %d)" % (what, n, len(q), len(t))
