"""BSDP's derived models of coding2genome on the device: the one-wave kernels of FAM_CODING2GENOME_START / _END / _JOIN and of the
six span families (three query rows per lane; START is the match state, the model's START or, in the span dst models, the intron
state) against the reference's records (tests/golden/derived_coding2genome*.jsonl, span_coding2genome_phase*.jsonl), against
refdump run on the spot at the strip and lane edges, as extra engines of a resident coding2genome batch, and in the heuristic
(BSDP) seam of the drop-in against the reference binary's recorded output.  No CPU oracle stands between (its split-codon calc is
the protein query's).  Integer work: every comparison is bit-exact."""
import ctypes as C
import random
import pytest

import exonerate_amd as ex
from exonerate_amd import _abi
import coding2genome_cases as cg
import coding2genome_derived_cases as cd

pytestmark = pytest.mark.gpu
needs_binaries = pytest.mark.skipif(not cd.HAVE_BINARIES, reason="reference binaries are built in the build container (make -C integration)")
needs_refdump = pytest.mark.skipif(not cd.HAVE_REFDUMP, reason="oracle/_ref/refdump is built by build() where the reference tree is")
LOW = _abi.IMPOSSIBLY_LOW_SCORE


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


def _check(name, recs, paths, scores):
    for rec, g, s in zip(recs, paths, scores):
        score, region, ops = cd.expected(rec)
        assert s["score"] == score, (name, rec["id"])
        if ops is not None:
            assert cd.of_result(g) == (score, region, ops), (name, rec["id"])


def _whole(recs):
    return [(r["query"], r["target"]) for r in recs], [{"pair": k, "region": (0, 0, len(r["query"]), len(r["target"]))} for k, r in enumerate(recs)]


# ---- the derived sets --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cd.SETS)
def test_every_record_as_a_single_job(eng, name):
    model = cd.set_model(name)
    recs = cd.records(name)
    paths, scores = [], []
    for rec in recs:
        q, t = rec["query"], rec["target"]
        job = [{"pair": 0, "region": (0, 0, len(q), len(t))}]
        paths += eng.viterbi(model, ex.MODE_FIND_PATH, [(q, t)], job)
        scores += eng.viterbi(model, ex.MODE_FIND_SCORE, [(q, t)], job)
    _check(name, recs, paths, scores)


@pytest.mark.parametrize("name", cd.SETS)
def test_every_record_of_a_set_in_one_launch(eng, name):
    model = cd.set_model(name)
    recs = cd.records(name)
    pairs, jobs = _whole(recs)
    _check(name, recs, eng.viterbi(model, ex.MODE_FIND_PATH, pairs, jobs), eng.viterbi(model, ex.MODE_FIND_SCORE, pairs, jobs))


# ---- the span seam -----------------------------------------------------------------------------------------------------
def _span_round(run_src, run_dst, phase, recs):
    """src DP (score, every END cell copied out, absent cells untouched), then the dst DP's score and path from those matrices:
    against records of refdump --cmd span.  run_src / run_dst(model, mode, pairs, jobs) launch."""
    src, dst = cd.span_src(phase), cd.span_dst(phase)
    cs = 1 + src.c.total_shadow_designations
    pairs, jobs = _whole(recs)
    mats = []
    for r, job in zip(recs, jobs):
        n = (len(r["query"]) + 1) * (len(r["target"]) + 1)
        m = (C.c_int32 * (n * cs))()
        for x in range(n):
            m[x * cs] = LOW
        mats.append(m)
        job["end_cells"] = m
    got = run_src(src, ex.MODE_FIND_SCORE, pairs, jobs)
    for r, g, m in zip(recs, got, mats):
        T = len(r["target"])
        assert g["score"] == r["src_score"], r["id"]
        exp = {(c[0], c[1]): c[2:] for c in r["end_cells"]}
        for i in range(len(r["query"]) + 1):
            for j in range(T + 1):
                x = (i * (T + 1) + j) * cs
                # (a cell the reference leaves out holds exactly -987654321: END is "set" there from an unset intron state, in
                # the reference's matrix as well, and its shadow slot is never read)
                assert [m[x + l] for l in range(cs)] == exp[(i, j)] if (i, j) in exp else m[x] == LOW, (r["id"], i, j)
    for job, m in zip(jobs, mats):
        del job["end_cells"]
        job["start_cells"] = m
    scores = run_dst(dst, ex.MODE_FIND_SCORE, pairs, jobs)
    paths = run_dst(dst, ex.MODE_FIND_PATH, pairs, jobs)
    for r, s_, p in zip(recs, scores, paths):
        assert s_["score"] == r["dst_score"], r["id"]
        if "path_score" in r:
            assert cd.of_result(p) == (r["path_score"], tuple(r["region"]), [tuple(o) for o in r["ops"]]), r["id"]
    return mats


@pytest.mark.parametrize("phase", range(3))
def test_span_seam_matches_reference_vectors(eng, phase):
    """viterbi.c:728-741, 793-799 at three rows per lane: every row of a lane that reaches END writes its own END cell, the dst
    DP reads its START cell per transition out of the intron state, and the start cell's shadow (with the base slot re-derived
    from it) travels through the split-codon post transition across lanes."""
    recs = cd.records(cd.SPAN_SETS[phase])
    _span_round(eng.viterbi, eng.viterbi, phase, recs)
    # the src traceback model (CORNER / CORNER, same tables): from the corner to the END cell the dst path started in.  refdump's
    # span records carry no src path, so what is held to the record is that path's score (the END cell's) and its corners
    tb = cd.span_src(phase, traceback=True)
    for r in recs:
        qe, te = r["region"][0], r["region"][1]
        got = eng.viterbi(tb, ex.MODE_FIND_PATH, [(r["query"], r["target"])], [{"pair": 0, "region": (0, 0, qe, te)}])[0]
        cell = [c for c in r["end_cells"] if (c[0], c[1]) == (qe, te)][0]
        assert got["score"] == cell[2] and (got["query_end"], got["target_end"]) == (qe, te), r["id"]


# ---- strip and lane edges, against refdump run on the spot -------------------------------------------------------------
@needs_refdump
def test_events_on_the_rows_around_a_lane_and_a_strip_edge(eng):
    """Whole small pairs in which a split codon's first row, a 3' exit or a frameshift sits on row 2, 3, 191, 192 or 193 of the
    rectangle, each with an intron of phase 0, 1 and 2 (45 pairs): the join model's score and path."""
    cases = cd.edge_cases()
    recs = cd.refdump_derived("join", cases)
    model = cd.all_models()["join"]
    for r in recs:                                              # (EDGE_SEED) every case, one by one
        a, ph, what = r["id"].split("_")
        assert (what, int(a[1:])) in cd.event_rows(model, r), r["id"]
        assert int(ph) in [p for p, _, _ in cg.introns_of(model, r["ops"], r["region"])], r["id"]
    pairs, jobs = _whole(recs)
    _check("edges", recs, eng.viterbi(model, ex.MODE_FIND_PATH, pairs, jobs), eng.viterbi(model, ex.MODE_FIND_SCORE, pairs, jobs))


@needs_refdump
@pytest.mark.parametrize("phase", range(3))
def test_span_seam_on_the_rows_around_a_lane_and_a_strip_edge(eng, phase):
    """The same pairs of this phase, the frameshift ones included, through the span seam: END cells of rows 191 ... 193 (the last lane of the first strip, the
    first of the second; rows past Q write nothing), start cells read there, the split codon's post transition across the edge."""
    cases = [c for c in cd.edge_cases() if c[0].split("_")[1] == str(phase)]
    recs = cd.refdump_span(phase, cases)
    assert len(recs) == 15 and all(cd.span_usable(r) for r in recs)
    assert sum(1 for r in recs if len(r["query"]) + 1 > cd.STRIP) >= 9
    for r in recs:                                              # the shift pairs: the frameshift lies in the src half of the span
        if r["id"].endswith("shift"):
            assert r["region"][0] > int(r["id"].split("_")[0][1:]), r["id"]
    _span_round(eng.viterbi, eng.viterbi, phase, recs)


def _fuzz_cases():
    rng = random.Random(cd.FUZZ_SEED)
    return [("f%02d" % k, ) + cd.fuzz_pair(rng) for k in range(60)]


@needs_refdump
@pytest.mark.parametrize("role", sorted(cd.ROLES))
def test_fuzz_of_small_pairs(eng, role):
    recs = cd.refdump_derived(role, _fuzz_cases())
    model = cd.all_models()[role]
    phases = [p for r in recs if "path_score" in r for p, _, _ in cg.introns_of(model, r["ops"], r["region"])]
    assert all(phases.count(p) >= 2 for p in range(3)), phases           # (FUZZ_SEED)
    pairs, jobs = _whole(recs)
    _check(role, recs, eng.viterbi(model, ex.MODE_FIND_PATH, pairs, jobs), eng.viterbi(model, ex.MODE_FIND_SCORE, pairs, jobs))


@needs_refdump
@pytest.mark.parametrize("phase", range(3))
def test_fuzz_of_small_pairs_through_the_span_seam(eng, phase):
    recs = [r for r in cd.refdump_span(phase, _fuzz_cases()) if r.get("end_cells")]
    assert len(recs) >= 40
    _span_round(eng.viterbi, eng.viterbi, phase, recs)


# ---- one launch of BSDP-sized jobs -------------------------------------------------------------------------------------
def _gene(rng, k):
    introns = [(8 + 14 * x, (k + x) % 3, rng.randint(30, 60)) for x in range(6)]
    return cg.gene_pair(rng, 100, introns=introns, events=[("q1", 30), ("t2", 58), ("qc", 75)], flank_t=0, sub=0.05, keep=2)


@needs_refdump
def test_two_thousand_bsdp_sized_jobs_in_one_launch(eng):
    """BSDP's unit of work -- rectangles of 1 ... 49 by 1 ... 120 -- as one launch of 2 000 join jobs, each a whole small pair cut
    out of a few gene pairs; every tenth against refdump run on the spot.  Then the same rectangles as sub-rectangles of the
    concatenated pair, through a resident coding2genome batch: the launch runs, and two submissions are equal (what a
    sub-rectangle must give -- splice context and the bases above its first row -- is the drop-in's check)."""
    rng = random.Random("coding2genome derived jobs")
    genes = [_gene(rng, k) for k in range(3)]
    model = cd.all_models()["join"]
    cuts = []
    for k in range(2000):
        g = k % 3
        q, t = genes[g]
        ql, tl = rng.randint(1, 49), rng.randint(1, 120)
        qs = rng.randint(0, len(q) - ql)
        ts = min(max(0, int(qs * len(t) / len(q)) + rng.randint(-20, 20)), len(t) - tl)
        cuts.append((g, qs, ts, ql, tl))
    pairs = [(genes[g][0][qs:qs + ql], genes[g][1][ts:ts + tl]) for g, qs, ts, ql, tl in cuts]
    jobs = [{"pair": k, "region": (0, 0, len(q), len(t))} for k, (q, t) in enumerate(pairs)]
    paths = eng.viterbi(model, ex.MODE_FIND_PATH, pairs, jobs)
    scores = eng.viterbi(model, ex.MODE_FIND_SCORE, pairs, jobs)
    sample = list(range(0, 2000, 10))
    recs = cd.refdump_derived("join", [("j%04d" % k, ) + pairs[k] for k in sample])
    _check("jobs", recs, [paths[k] for k in sample], [scores[k] for k in sample])
    assert sum(1 for r in recs if "path_score" in r and cg.introns_of(model, r["ops"], r["region"])) >= 10
    qcat, tcat = "".join(g[0] for g in genes), "".join(g[1] for g in genes)
    qoff = [0, len(genes[0][0]), len(genes[0][0]) + len(genes[1][0])]
    toff = [0, len(genes[0][1]), len(genes[0][1]) + len(genes[1][1])]
    sub = [{"pair": 0, "region": (qoff[g] + qs, toff[g] + ts, ql, tl)} for g, qs, ts, ql, tl in cuts]
    batch = ex.ResidentBatch(eng, ex.Model("coding2genome"), [(qcat, tcat)])
    try:
        first = batch.viterbi(ex.MODE_FIND_PATH, sub, model=model)
        again = batch.viterbi(ex.MODE_FIND_PATH, sub, model=model)
        s1 = batch.viterbi(ex.MODE_FIND_SCORE, sub, model=model)
    finally:
        batch.close()
    assert [cd.of_result(g) for g in first] == [cd.of_result(g) for g in again]
    assert [g["score"] for g in s1] == [g["score"] for g in first]


def test_span_models_on_a_resident_coding2genome_batch(eng):
    """c4gpu_batch_viterbi_model with start_cells / end_cells: the span engines read the batch's codon row codes, forward splice
    arrays, base masks and intron limits -- the recorded span pairs as pairs of one resident batch."""
    for phase in range(3):
        recs = cd.records(cd.SPAN_SETS[phase])
        batch = ex.ResidentBatch(eng, ex.Model("coding2genome"), [(r["query"], r["target"]) for r in recs])
        try:
            run = lambda model, mode, pairs, jobs: batch.viterbi(mode, jobs, model=model)       # noqa: E731
            _span_round(run, run, phase, recs)
        finally:
            batch.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_derived_models_do_not_cross_batches(eng, capfd, monkeypatch):
    """coding2genome's derived models on a coding2coding or est2genome batch, and coding2coding's on a coding2genome batch, are
    refused with the batch's error before anything is launched."""
    monkeypatch.setenv("C4GPU_TRACE", "1")
    q, t = cg.gene_pair(random.Random(5), 20, introns=[(9, 1, 40)], flank_t=0)
    job = [{"pair": 0, "region": (3, 3, 30, 60)}]
    c2g_join, c2c_join = ex.Model.derived("coding2genome", 2, 2, 4, 4), ex.Model.derived("coding2coding", 2, 2, 4, 4)
    for batch_type, others in (("coding2coding", [c2g_join, cd.span_src(1)]), ("est2genome", [c2g_join, cd.span_dst(2)]),
                               ("coding2genome", [c2c_join])):
        batch = ex.ResidentBatch(eng, ex.Model(batch_type), [(q, t)])
        try:
            for other in others:
                capfd.readouterr()
                with pytest.raises(Exception, match="needs sequence arrays this batch was not built with"):
                    batch.viterbi(ex.MODE_FIND_SCORE, job, model=other)
                assert "c4gpu trace:   kernel " not in capfd.readouterr().err
        finally:
            batch.close()


# ---- nothing reads a buffer before it is written -----------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["90", "255"])
def test_nothing_depends_on_what_a_new_buffer_held(eng, monkeypatch, fill):
    monkeypatch.setenv("C4GPU_FILL_ALLOC", fill)
    for phase in range(3):
        _span_round(eng.viterbi, eng.viterbi, phase, cd.records(cd.SPAN_SETS[phase]))
    name = "derived_coding2genome_join"
    recs = cd.records(name)
    pairs, jobs = _whole(recs)
    _check(name, recs, eng.viterbi(cd.set_model(name), ex.MODE_FIND_PATH, pairs, jobs),
           eng.viterbi(cd.set_model(name), ex.MODE_FIND_SCORE, pairs, jobs))


# ---- the drop-in on the device -----------------------------------------------------------------------------------------
@needs_binaries
@pytest.mark.parametrize("variant", sorted(cd.CLI_VARIANTS))
def test_heuristic_coding2genome_runs_its_sub_dps_in_device_batches(tmp_path, variant):
    data = cd.load_cli()
    extra = cd.CLI_REPORTS + cd.CLI_VARIANTS[variant]
    _, gpu, err = cd.run_pair(tmp_path, "coding2genome", extra, {"C4GPU_CODING2GENOME_BSDP": "1"}, inputs=cd.cli_inputs(), ref=False)
    assert cd.stable_lines(gpu) == cd.cli_stdout(data, variant)
    assert "has no device family" not in err and "stay on the CPU" not in err, err[-1500:]
    got = cd.served(err)
    assert got, err[-1500:]
    s_ok, s_all, p_ok, p_all = got
    print("served: %d of %d score calls, %d of %d path calls" % (s_ok, s_all, p_ok, p_all))
    assert int(err.split(" spans) in device batches")[0].rsplit("(", 1)[1]) > 0, err[-600:]
    assert s_all > 0 and p_all > 0
    if variant == "S_no":
        assert (s_ok, p_ok) == (s_all, p_all), err[-600:]
    else:
        assert s_ok + p_ok >= 0.7 * (s_all + p_all), err[-600:]
    if variant.startswith("refine"):
        assert cd.refinements(err), err[-800:]


def _check_line(err):
    import re
    m = re.search(r"c4gpu bsdp: check (\d+) candidates, (\d+) mismatches", err)
    assert m, err[-1500:]
    return int(m.group(1)), int(m.group(2))


@needs_binaries
def test_the_reference_recomputes_every_device_answer(tmp_path):
    """C4GPU_BSDP_CHECK=1: at the flush every candidate the device answered -- terminals, joins, the spans' src / dst / src
    traceback DPs, on SUB-rectangles of the long sequences, with the splice sites' context and the bases above a region's first
    row -- is computed again by the reference's own Optimal_find_score / Optimal_find_path; none may differ."""
    data = cd.load_cli()
    _, gpu, err = cd.run_pair(tmp_path, "coding2genome", cd.CLI_REPORTS, {"C4GPU_CODING2GENOME_BSDP": "1", "C4GPU_BSDP_CHECK": "1"},
                              inputs=cd.cli_inputs(), ref=False)
    assert cd.stable_lines(gpu) == cd.cli_stdout(data, "default")
    n, bad = _check_line(err)
    assert n > 0 and bad == 0, err[-1500:]
    # off: no such line
    _, _, err = cd.run_pair(tmp_path, "coding2genome", cd.CLI_REPORTS, {"C4GPU_CODING2GENOME_BSDP": "1"}, inputs=cd.cli_inputs(), ref=False)
    assert "c4gpu bsdp: check" not in err


@needs_binaries
@pytest.mark.parametrize("model", ["est2genome", "protein2genome"])
def test_the_check_mode_where_the_seam_is_known_to_hold(tmp_path, model):
    from test_integration_bsdp_host import heuristic_inputs
    _, gpu, err = cd.run_pair(tmp_path, model, [], {"C4GPU_BSDP_CHECK": "1"}, inputs=heuristic_inputs(model, 4, 5), ref=False)
    assert gpu.count(b"vulgar:") >= 4
    n, bad = _check_line(err)
    assert n > 0 and bad == 0, err[-1500:]
