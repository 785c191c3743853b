"""BSDP's derived models of coding2coding on the device: the one-wave kernels of FAM_CODING2CODING_START / _END / _JOIN (three
query rows per lane; transitions leave START with a query advance of 1, 2 and 3) against the reference's records
(tests/golden/derived_coding2coding*.jsonl) and the oracle, on their own and as extra engines of a resident coding2coding batch,
and the heuristic (BSDP) seam of the drop-in against the reference binary.  Integer work: every comparison is bit-exact."""
import random
import pytest

import exonerate_amd as ex
import codon_cases as cc
import codon_derived_cases as cd

pytestmark = pytest.mark.gpu
needs_binaries = pytest.mark.skipif(not cd.HAVE_BINARIES, reason="reference binaries are built in the build container (make -C integration)")


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
    pairs = [(r["query"], r["target"]) for r in recs]
    jobs = [{"pair": k, "region": (0, 0, len(r["query"]), len(r["target"]))} for k, r in enumerate(recs)]
    _check(name, recs, eng.viterbi(model, ex.MODE_FIND_PATH, pairs, jobs), eng.viterbi(model, ex.MODE_FIND_SCORE, pairs, jobs))


def _homologous_pair(rng, ncod=500):
    """One coding pair of about 1 500 bases with a planted event every forty codons or so."""
    qc, tc = cc._homologous(rng, [rng.choice(cc.AA) for _ in range(ncod)])
    for at in range(20, ncod, 40):
        kind = rng.choice(sorted(cc.EVENT_SHAPE))
        side = qc if kind[0] == "q" else tc
        side[at] += cc._dna(rng, {"1": 1, "2": 2, "c": 3}[kind[1]])
    return "".join(qc), "".join(tc) + cc._dna(rng, 300)


@pytest.mark.parametrize("role", sorted(cd.ROLES))
def test_thousands_of_bsdp_sized_jobs(eng, role):
    """BSDP's unit of work -- rectangles of 1 ... 49 by 1 ... 49 of ONE pair -- as one launch of 3 000 jobs per derived model
    (the shape of test_thousands_of_bsdp_sized_jobs_on_derived_models); every seventh job against the oracle."""
    rng = random.Random("codon derived jobs " + role)
    q, t = _homologous_pair(rng)
    model = ex.Model.derived("coding2coding", *cd.ROLES[role])
    jobs = []
    for k in range(3000):
        ql, tl = rng.randint(1, 49), rng.randint(1, 49)
        qs = rng.randint(0, len(q) - ql)
        ts = min(max(0, qs + rng.randint(-10, 10)), len(t) - tl) if k % 2 else rng.randint(0, len(t) - tl)
        jobs.append({"pair": 0, "region": (qs, ts, ql, tl)})
    got = eng.viterbi(model, ex.MODE_FIND_PATH, [(q, t)], jobs)
    scores = eng.viterbi(model, ex.MODE_FIND_SCORE, [(q, t)], jobs)
    for k in range(0, len(jobs), 7):
        exp = cd.oracle(model, ex.MODE_FIND_PATH, q, t, jobs[k]["region"])
        assert cd.of_result(got[k]) == exp, (role, jobs[k])
        assert scores[k]["score"] == exp[0], (role, jobs[k])


def test_derived_models_on_a_resident_coding2coding_batch(eng):
    """c4gpu_batch_viterbi_model: the derived models' engines read the sequence arrays of the batch's own model, among them the
    per-position translated query codes that a codon batch builds once per unique query -- here two pairs share one query buffer
    and a third has its own."""
    rng = random.Random("codon derived batch")
    q1, t1 = _homologous_pair(rng, 120)
    q2, t2 = _homologous_pair(rng, 90)
    _, t3 = _homologous_pair(rng, 120)
    t3 = t1[:150] + t3[150:]
    pairs = [(q1, t1), (q2, t2), (q1, t3)]                      # (one str object in two pairs: one buffer, _pairs)
    batch = ex.ResidentBatch(eng, ex.Model("coding2coding"), pairs)
    try:
        for role, spec in sorted(cd.ROLES.items()):
            model = ex.Model.derived("coding2coding", *spec)
            jobs = []
            for k in range(240):
                p = k % 3
                q, t = pairs[p]
                ql, tl = rng.randint(1, 49), rng.randint(1, 49)
                qs = rng.randint(0, len(q) - ql)
                jobs.append({"pair": p, "region": (qs, min(max(0, qs + rng.randint(-6, 6)), len(t) - tl), ql, tl)})
            got = batch.viterbi(ex.MODE_FIND_PATH, jobs, model=model)
            scores = batch.viterbi(ex.MODE_FIND_SCORE, jobs, model=model)
            for k in range(0, len(jobs), 4):
                q, t = pairs[jobs[k]["pair"]]
                exp = cd.oracle(model, ex.MODE_FIND_PATH, q, t, jobs[k]["region"])
                assert cd.of_result(got[k]) == exp and scores[k]["score"] == exp[0], (role, jobs[k])
    finally:
        batch.close()


def test_codon_and_plain_models_do_not_share_a_batch(eng, capfd, monkeypatch):
    """A codon derived model needs the translated query codes an affine batch never built, and an affine derived model cannot
    read a codon batch's: both are refused with an error, before anything is launched."""
    monkeypatch.setenv("C4GPU_TRACE", "1")
    q, t = _homologous_pair(random.Random(5), 40)
    job = [{"pair": 0, "region": (3, 3, 30, 30)}]
    for batch_type, other in (("affine:local", "coding2coding"), ("coding2coding", "affine:local")):
        batch = ex.ResidentBatch(eng, ex.Model(batch_type), [(q, t)])
        try:
            capfd.readouterr()
            with pytest.raises(Exception, match="needs sequence arrays this batch was not built with"):
                batch.viterbi(ex.MODE_FIND_SCORE, job, model=ex.Model.derived(other, 2, 2, 4, 4))
            assert "c4gpu trace:   kernel " not in capfd.readouterr().err
            own = ex.Model.derived(batch_type, 2, 2, 4, 4)      # ... and the batch still serves its own derived model
            assert batch.viterbi(ex.MODE_FIND_SCORE, job, model=own)[0]["score"] == \
                cd.oracle(own, ex.MODE_FIND_SCORE, q, t, job[0]["region"])[0]
        finally:
            batch.close()


# ---- the drop-in on the device -----------------------------------------------------------------------------------------
@needs_binaries
@pytest.mark.parametrize("extra", [[], ["-S", "no"], ["--refine", "region"], ["--refine", "full", "--bestn", "1"]],
                         ids=["default", "S_no", "refine_region", "refine_full_bestn1"])
def test_heuristic_coding2coding_runs_its_sub_dps_in_device_batches(tmp_path, extra):
    ref, gpu, err = cd.run_pair(tmp_path, "coding2coding", extra, {})
    assert gpu == ref
    assert ref.count(b"vulgar:") >= 4
    assert "has no device family" not in err and "stay on the CPU" not in err, err[-1500:]
    got = cd.served(err)
    assert got, err[-1500:]
    s_ok, s_all, p_ok, p_all = got
    print("served: %d of %d score calls, %d of %d path calls" % (s_ok, s_all, p_ok, p_all))
    assert s_all > 0 and p_all > 0
    if "-S" in extra:
        assert (s_ok, p_ok) == (s_all, p_all), err[-600:]
    else:
        assert s_ok + p_ok >= 0.7 * (s_all + p_all), err[-600:]
    if "--refine" in extra:
        assert cd.refinements(err), err[-800:]
