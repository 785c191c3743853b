"""exonerate's --annotation (match.c:276-281: no 1:1 DNA match inside the query's CDS) on every entry point of a resident batch.

c4gpu_batch_set_annotation changes the query codes on the device, the engine's parameter block and the set of kernels that may
run -- for every later call on the batch.  Here each of those calls runs under an annotation: the score, region and path passes,
the sub-optimal loop, run_regions, the raw Viterbi modes, the derived models of c4gpu_batch_viterbi_model, both memory routes
on queries of several strips, swap_stage, pairs that share a query buffer, and the models the veto does not concern.  Yardsticks:
the reference's own annotated records (tests/golden/*_annot*.jsonl) and, for seeded inputs (annot_cases.py, shown to be decided by
the annotation in test_annot_cases.py), the CPU oracle under oracle_set_annotation.  Integer work: every comparison is exact.

While a DNA annotation is armed no kernel with the local-scope shortcut (`_local`) and no packed 16-bit kernel (`pk16`, `16_`) may
run: a match score of -987654321 is outside their guards.  The launched names come from C4GPU_TRACE."""
import random
import re

import pytest

import exonerate_amd as ex
from exonerate_amd import _abi
import annot_cases as ac
import ner_cases
from golden_util import ANNOT_SETS, ANNOT_SUBOPT_SETS, load_set, expected, set_params, set_spec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _oracle_without_annotation():
    """A test that fails inside an annotated oracle call must not leave the annotation to the tests after it."""
    yield
    import oracle_lib
    oracle_lib.set_annotation(None)


def _kernels(capfd):
    """names of the kernels launched since the last look: `c4gpu trace:   kernel <name>: <n> workgroups per CU` of the engine's
    launches, and the lines of the device route through the reduced-space steps, which launches its kernels itself
    (`fused: kernels <checkpoint>, <path>` / `fused: packed checkpoint kernels <name or -> for <n>, <name or -> for <n> of <n> jobs`)"""
    err = capfd.readouterr().err
    names = re.findall(r"c4gpu trace:   kernel (\w+):", err)
    for pair in re.findall(r"c4gpu trace:   fused: kernels (\w+), (\w+)", err):
        names += pair
    for pair in re.findall(r"c4gpu trace:   fused: packed checkpoint kernels (\S+) for \d+, (\S+) for \d+ of", err):
        names += [n for n in pair if n != "-"]
    return names


def _assert_guarded(names):
    assert names and not any("_local" in n or "pk16" in n or "16_" in n for n in names), names


def _set_model(name):
    if name in ner_cases.ANNOT_SETS or name in ner_cases.REFDUMP_SETS:
        return ner_cases.open0_model(name)
    mt, qa, ta = set_spec(name)
    return ex.Model(mt, qa, ta, params=set_params(_abi.load(), name))


def _dict(aln, qid="qy"):
    return aln.as_dict(qid) if aln is not None else None


def _passes(b, recs, dpm):
    """every pass of the batch: (scores of run(0), scores and regions of run(1), alignments of run(2))"""
    b.run(0)
    s0 = b.scores()[0]
    b.run(1)
    s1, r1 = b.scores()
    b.run(2, dpmemory=dpm)
    return s0, s1, [list(r) for r in r1], [_dict(b.alignment(i), r["id"]) for i, r in enumerate(recs)]


def _assert_records(got, recs):
    s0, s1, r1, alns = got
    assert s0 == [r["score"] for r in recs]
    assert s1 == [r["score"] for r in recs]
    for rec, region, aln in zip(recs, r1, alns):
        if "path_score" not in rec:
            assert aln is None, rec["id"]
            continue
        assert region == rec["region"], rec["id"]
        assert aln == expected(rec), rec["id"]


@pytest.mark.parametrize("name", sorted(ANNOT_SETS) + sorted(ner_cases.ANNOT_SETS))
def test_reference_sets_through_every_pass(eng, name, monkeypatch, capfd):
    """The reference's annotated records through run(0), run(1) and run(2); the annotation taken away restores the plain
    results; an annotation that replaces another one (the codes are first written again from the residues) gives the records."""
    model = _set_model(name)
    recs = load_set(name)
    cds = [tuple(r["cds"]) for r in recs]
    dpm = recs[0]["dpmemory"]
    monkeypatch.setenv("C4GPU_TRACE", "1")
    b = ex.ResidentBatch(eng, model, [(r["query"], r["target"]) for r in recs])
    plain = _passes(b, recs, dpm)
    capfd.readouterr()
    b.set_annotation(cds)
    got = _passes(b, recs, dpm)
    _assert_guarded(_kernels(capfd))
    _assert_records(got, recs)
    assert sum(a != p for a, p in zip(got[3], plain[3])) >= len(recs) // 3
    b.set_annotation(None)
    assert _passes(b, recs, dpm) == plain
    b.set_annotation([(s + 3, l + 2) for s, l in cds])              # another annotation in between ...
    b.set_annotation(cds)                                           # ... replaced: nothing of it may stay
    assert _passes(b, recs, dpm) == got
    b.set_annotation(cds)                                           # and the same one set twice
    assert _passes(b, recs, dpm) == got
    b.close()


@pytest.mark.parametrize("name", sorted(ANNOT_SUBOPT_SETS))
def test_suboptimal_loop_under_an_annotation(eng, name, monkeypatch, capfd):
    """run(2) and next_paths rounds with the annotation armed: the veto and the SubOpt blocking in the same cells (the `_sub`
    kernels), against the successive alignments the reference produced with the annotation attached."""
    model = _set_model(name)
    recs = load_set(name)
    dpm, thr = recs[0]["dpmemory"], recs[0]["threshold"]
    monkeypatch.setenv("C4GPU_TRACE", "1")
    b = ex.ResidentBatch(eng, model, [(r["query"], r["target"]) for r in recs])
    b.set_annotation([tuple(r["cds"]) for r in recs])
    capfd.readouterr()
    b.run(2, dpm, thr)
    rounds = [[b.alignment(i) for i in range(len(recs))]]
    while len(rounds) < 4 and b.next_paths(dpm, thr) > 0:           # --suboptmax 4
        rounds.append([b.alignment(i) for i in range(len(recs))])
    names = _kernels(capfd)
    b.close()
    _assert_guarded(names)
    assert any(n.endswith("_sub") for n in names), names
    assert sum(len(r["subopt"]) for r in recs) > len(recs)          # the loop went round
    for i, rec in enumerate(recs):
        got = [r[i] for r in rounds if r[i] is not None]
        assert [(a.score, list(a.region), [list(o) for o in a.ops], a.vulgar(rec["id"])) for a in got] == \
               [(e["path_score"], e["region"], e["ops"], e["vulgar"]) for e in rec["subopt"]], rec["id"]


def _assert_jobs(got, exp, mode, tag):
    assert len(got) == len(exp)
    for k, (g, e) in enumerate(zip(got, exp)):
        if mode == ex.MODE_FIND_SCORE:
            assert g["score"] == e["score"], (tag, k)
        else:
            keys = ("score", "query_start", "target_start", "query_end", "target_end", "ops")
            assert [g[x] for x in keys] == [e[x] for x in keys], (tag, k)


@pytest.mark.parametrize("index", range(len(ac.DERIVED_MODELS)))
def test_derived_models_on_an_annotated_batch(eng, index, monkeypatch, capfd):
    """BSDP's terminal and join sub-DPs (c4gpu_batch_viterbi_model) read the batch's query codes: on an annotated batch their
    engines arm the same veto row, whether they were made before the annotation was set or after it.  Every job of ~300, score
    and path, against oracle_viterbi under the annotation."""
    mt, spec = ac.DERIVED_MODELS[index]
    base, drv = ex.Model(mt), ex.Model.derived(mt, *spec)
    q, t, jobs = ac.derived_case()
    plain, annot = ac.derived_oracle(index, False), ac.derived_oracle(index, True)
    modes = (ex.MODE_FIND_SCORE, ex.MODE_FIND_PATH)
    monkeypatch.setenv("C4GPU_TRACE", "1")
    # (a) the extra engine exists before the annotation is set
    b = ex.ResidentBatch(eng, base, [(q, t)])
    for mode in modes:
        _assert_jobs(b.viterbi(mode, jobs, model=drv), plain, mode, "plain, before")
    b.set_annotation([ac.DERIVED_CDS])
    capfd.readouterr()
    for mode in modes:
        _assert_jobs(b.viterbi(mode, jobs, model=drv), annot, mode, "annotated, engine made before")
    _assert_guarded(_kernels(capfd))
    # (c) and after the annotation is taken away
    b.set_annotation(None)
    for mode in modes:
        _assert_jobs(b.viterbi(mode, jobs, model=drv), plain, mode, "plain, after")
    b.close()
    # (b) the annotation first
    b = ex.ResidentBatch(eng, base, [(q, t)])
    b.set_annotation([ac.DERIVED_CDS])
    for mode in modes:
        _assert_jobs(b.viterbi(mode, jobs, model=drv), annot, mode, "annotated first")
    b.close()


def test_raw_viterbi_modes_on_an_annotated_batch(eng, monkeypatch, capfd):
    """Viterbi_DP_Func level on the batch's own model: the region pass and a checkpoint pass with a START -> END continuation."""
    model = ex.Model("est2genome")
    rng = random.Random(5)
    q = ac._rand(rng, 150)
    t = ac._rand(rng, 60) + q[:70] + "GT" + ac._rand(rng, 300) + "AG" + q[70:] + ac._rand(rng, 80)
    cds = (100, 6)                     # short enough for the best path to bridge it with a pair of gaps
    region = (0, 0, len(q), len(t))
    keys = ("score", "query_start", "target_start", "query_end", "target_end")
    with ac.oracle_annotation(None):
        plain = ac.oracle_job(model, ex.MODE_FIND_REGION, q, t, region)
    with ac.oracle_annotation(cds):
        exp = ac.oracle_job(model, ex.MODE_FIND_REGION, q, t, region)
    assert [exp[k] for k in keys] != [plain[k] for k in keys]
    monkeypatch.setenv("C4GPU_TRACE", "1")
    b = ex.ResidentBatch(eng, model, [(q, t)])
    b.set_annotation([cds])
    capfd.readouterr()
    got = b.viterbi(ex.MODE_FIND_REGION, [{"pair": 0, "region": region}])[0]
    assert [got[k] for k in keys] == [exp[k] for k in keys]
    ar = (exp["query_start"], exp["target_start"], exp["query_end"] - exp["query_start"], exp["target_end"] - exp["target_start"])
    cont = _abi.Continuation()
    cont.first_state, cont.final_state = model.c.start_state, model.c.end_state
    with ac.oracle_annotation(cds):
        exp = ac.oracle_job(model, ex.MODE_FIND_CHECKPOINTS, q, t, ar, cont, 5)
    with ac.oracle_annotation(None):
        plain = ac.oracle_job(model, ex.MODE_FIND_CHECKPOINTS, q, t, ar, cont, 5)
    assert exp["score"] != plain["score"]
    got = b.viterbi(ex.MODE_FIND_CHECKPOINTS, [{"pair": 0, "region": ar, "checkpoints": 5,
                                                "continuation": {"first_state": model.c.start_state,
                                                                 "final_state": model.c.end_state}}])[0]
    assert (got["score"], got["last_srp"]) == (exp["score"], exp["last_srp"])
    # slot 1 (intron shadow) of a non-intron state is never read again: the engine reports 0 there
    assert [got["final_cell"][0], got["final_cell"][exp["cell_size"] - 1]] == exp["final_cell"]
    _assert_guarded(_kernels(capfd))
    b.close()


@pytest.mark.parametrize("dpm", [32, 1])
@pytest.mark.parametrize("name", [m[0] for m in ac.LONG_MODELS])
def test_long_queries_under_an_annotation(eng, name, dpm, monkeypatch, capfd):
    """Queries past two strips of 64 x R rows, every CDS variant in one batch (each on a query buffer of its own): the quadratic
    route at -D 32, checkpoints and continuation sub-alignments at -D 1.  The 520 nt affine:local query has three strips: its
    score and region passes must be the cooperating-wave kernels without the local-scope shortcut."""
    model, q, t = ac.long_case(name)
    variants = [cds for cds, _ in ac.long_cds_variants(len(q))]
    changes = dict(ac.long_cds_variants(len(q)))                   # (a CDS outside the query: the oracle's plain result)
    pairs = [(bytes(bytearray(q.encode())), t) for _ in variants]
    monkeypatch.setenv("C4GPU_TRACE", "1")
    b = ex.ResidentBatch(eng, model, pairs)
    b.set_annotation(variants)
    capfd.readouterr()
    b.run(2, dpmemory=dpm)
    names = _kernels(capfd)
    _assert_guarded(names)
    if dpm == 1:
        assert any("ckpt" in n for n in names) and any("cont" in n for n in names), names
    for i, cds in enumerate(variants):
        assert _dict(b.alignment(i)) == ac.long_oracle(name, cds if changes[cds] else None, dpm), (name, cds)
    if dpm == 32 and name in ac.LONG_KERNELS:
        # three strips of 256 rows in every job: the score and region passes are the cooperating-wave kernels' (the 32-bit ones
        # without the local-scope shortcut, which nothing but an annotation or out-of-range parameters selects); their scores
        # and regions are the oracle's, with the packed region-start slot and with the two-slot form (C4GPU_PACK=0)
        exp = [ac.long_oracle(name, cds if changes[cds] else None, dpm) for cds in variants]
        b.run(0)
        assert b.scores()[0] == [e["score"] for e in exp]
        b.run(1)
        assert [(s, list(r)) for s, r in zip(*b.scores())] == [(e["score"], e["region"]) for e in exp]
        names += _kernels(capfd)
        monkeypatch.setenv("C4GPU_PACK", "0")
        b.run(1)
        assert [(s, list(r)) for s, r in zip(*b.scores())] == [(e["score"], e["region"]) for e in exp]
        unpacked = _kernels(capfd)
        monkeypatch.delenv("C4GPU_PACK")
        _assert_guarded(names + unpacked)
        assert all(k in names for k in ac.LONG_KERNELS[name]), names
        assert "kmw_affine_region" in unpacked, unpacked
    b.set_annotation(None)
    b.run(2, dpmemory=dpm)
    for i in range(len(variants)):
        assert _dict(b.alignment(i)) == ac.long_oracle(name, None, dpm)
    b.close()


@pytest.mark.parametrize("dpm", [32, 1])
def test_run_regions_under_an_annotation(eng, dpm, monkeypatch, capfd):
    """--refine region's call with regions that cut through the CDS, one pair switched off."""
    model = ex.Model("est2genome")
    cases = ac.region_cases()
    active = [k != 2 for k in range(len(cases))]
    monkeypatch.setenv("C4GPU_TRACE", "1")
    b = ex.ResidentBatch(eng, model, [(q, t) for q, t, _, _ in cases])
    b.set_annotation([cds for _, _, cds, _ in cases])
    capfd.readouterr()
    b.run_regions([r for _, _, _, r in cases], dpmemory=dpm, active=active)
    _assert_guarded(_kernels(capfd))
    for i, (q, t, cds, region) in enumerate(cases):
        if not active[i]:
            assert b.alignment(i) is None
            continue
        assert _dict(b.alignment(i)) == ac.oracle_path(model, q, t, cds, dpm, region), i
    b.close()


def _shared_case():
    rng = random.Random(616)
    q = ac._rand(rng, 150)
    targets = [ac._rand(rng, 20 + 7 * k) + ac._mutate(rng, q, 0.05) + ac._rand(rng, 30) for k in range(3)]
    return q, targets


def _run2(b, n):
    b.run(2)
    return [_dict(b.alignment(i)) for i in range(n)]


def test_shared_query_buffer_same_annotation(eng):
    """One query object against three targets is one copy of the query on the device: the same annotation on all three."""
    model = ex.Model("affine:local")
    q, targets = _shared_case()
    cds = (50, 40)
    qb = q.encode()
    b = ex.ResidentBatch(eng, model, [(qb, t) for t in targets])
    b.set_annotation([cds] * 3)
    exp = [ac.oracle_path(model, q, t, cds) for t in targets]
    assert _run2(b, 3) == exp
    assert exp != [ac.oracle_path(model, q, t, None) for t in targets]
    b.close()


def test_shared_query_buffer_refuses_differing_annotations(eng):
    """Pairs that share a query buffer cannot carry different annotations, "none" included (the codes are shared): the call is
    refused, says why, and leaves the batch as it was -- un-annotated or with the annotation it had."""
    lib = _abi.load()
    model = ex.Model("affine:local")
    q, targets = _shared_case()
    cds = (50, 40)
    qb = q.encode()
    b = ex.ResidentBatch(eng, model, [(qb, t) for t in targets])
    plain = [ac.oracle_path(model, q, t, None) for t in targets]
    annot = [ac.oracle_path(model, q, t, cds) for t in targets]
    assert _run2(b, 3) == plain
    for bad in ([cds, (10, 20), cds], [cds, None, cds], [None, None, (50, 40)]):
        with pytest.raises(ex.C4GpuError):
            b.set_annotation(bad)
        err = lib.c4gpu_last_error()
        assert b"c4gpu_batch_set_annotation" in err and b"share a query buffer" in err, err
        assert _run2(b, 3) == plain, bad                            # nobody inherits a neighbour's annotation
    b.set_annotation([cds] * 3)
    assert _run2(b, 3) == annot
    with pytest.raises(ex.C4GpuError):
        b.set_annotation([cds, (10, 20), cds])
    assert _run2(b, 3) == annot                                     # the annotation from before the refused call
    b.close()


def test_empty_query_shares_no_buffer(eng):
    """An empty query takes no room among the codes, so the query after it begins at the same offset: the two share nothing,
    and whatever annotation the empty one is given, the other keeps its own."""
    model = ex.Model("affine:local")
    q, targets = _shared_case()
    cds = (50, 40)
    region = (0, 0, len(q), len(targets[1]))
    with ac.oracle_annotation(cds):
        exp = ac.oracle_job(model, ex.MODE_FIND_PATH, q, targets[1], region)
    with ac.oracle_annotation(None):
        assert exp["score"] != ac.oracle_job(model, ex.MODE_FIND_PATH, q, targets[1], region)["score"]
    b = ex.ResidentBatch(eng, model, [(b"", targets[0]), (q, targets[1])])
    keys = ("score", "query_start", "target_start", "query_end", "target_end", "ops")
    for first in (None, (0, 5)):
        b.set_annotation([first, cds])
        got = b.viterbi(ex.MODE_FIND_PATH, [{"pair": 1, "region": region}])[0]
        assert [got[k] for k in keys] == [exp[k] for k in keys], first
    b.close()


def test_equal_queries_in_buffers_of_their_own(eng):
    """The same residues as three distinct objects: three copies on the device, three annotations."""
    model = ex.Model("affine:local")
    q, targets = _shared_case()
    cds = [(50, 40), (10, 20), None]
    b = ex.ResidentBatch(eng, model, [(bytes(bytearray(q.encode())), t) for t in targets])
    b.set_annotation(cds)
    exp = [ac.oracle_path(model, q, t, c) for t, c in zip(targets, cds)]
    assert _run2(b, 3) == exp
    assert len({e["score"] for e in (ac.oracle_path(model, q, targets[0], c) for c in cds)}) == 3     # three different answers
    b.close()


@pytest.mark.parametrize("name", ["affine_local_protein", "protein2dna", "ner_protein_open0"])
def test_models_without_a_dna_match_are_left_alone(eng, name, monkeypatch, capfd):
    """The veto belongs to the 1:1 DNA match calc: a batch whose model has none accepts the call and changes nothing -- the
    reference's records before and after, and the same kernels (the local-scope shortcut and the packed passes stay)."""
    model = _set_model(name)
    recs = load_set(name)
    dpm = recs[0]["dpmemory"]
    monkeypatch.setenv("C4GPU_TRACE", "1")
    b = ex.ResidentBatch(eng, model, [(r["query"], r["target"]) for r in recs])
    capfd.readouterr()
    before = _passes(b, recs, dpm)
    names = sorted(_kernels(capfd))
    _assert_records(before, recs)
    assert any("_local" in n for n in names), names
    b.set_annotation([(len(r["query"]) // 3, max(1, len(r["query"]) // 3)) for r in recs])       # success: no exception
    capfd.readouterr()
    after = _passes(b, recs, dpm)
    assert sorted(_kernels(capfd)) == names
    _assert_records(after, recs)
    b.close()


def test_swap_stage_and_annotations(eng, monkeypatch, capfd):
    """An annotation belongs to the sequences the batch holds: staged pairs come in without one (their codes are the residues'),
    take their own, lose it again; the buffers handed back to the stage with annotated codes are written anew by its next load."""
    model = ex.Model("est2genome")
    sets = [ac.est_pairs(seed, 6) for seed in (5151, 5152, 5153)]

    def oracle(pairs, annotated):
        return [ac.oracle_path(model, q, t, cds if annotated else None) for q, t, cds in pairs]

    monkeypatch.setenv("C4GPU_TRACE", "1")
    b = ex.ResidentBatch(eng, model, [(q, t) for q, t, _ in sets[0]])
    b.set_annotation([cds for _, _, cds in sets[0]])
    capfd.readouterr()
    assert _run2(b, 6) == oracle(sets[0], True)
    _assert_guarded(_kernels(capfd))
    stage = ex.Stage(eng, model)
    stage.load([(q, t) for q, t, _ in sets[1]])
    b.swap(stage)
    assert _run2(b, 6) == oracle(sets[1], False)
    b.set_annotation([cds for _, _, cds in sets[1]])
    capfd.readouterr()
    assert _run2(b, 6) == oracle(sets[1], True)
    _assert_guarded(_kernels(capfd))
    b.set_annotation(None)
    assert _run2(b, 6) == oracle(sets[1], False)
    b.set_annotation([cds for _, _, cds in sets[1]])
    stage.load([(q, t) for q, t, _ in sets[2]])                     # into the buffers that held the first, annotated set
    b.swap(stage)
    assert _run2(b, 6) == oracle(sets[2], False)
    b.set_annotation([cds for _, _, cds in sets[2]])
    assert _run2(b, 6) == oracle(sets[2], True)
    b.set_annotation(None)
    assert _run2(b, 6) == oracle(sets[2], False)
    stage.close()
    b.close()
