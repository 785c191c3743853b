"""Pin the oracle (oracle/c4_oracle.c) against outputs of the REFERENCE ITSELF.

tests/golden/*.jsonl were produced by tools/make_golden.py running oracle/_ref/refdump, i.e. the
reference's own Optimal_find_score / Optimal_find_path (interpreted Viterbi) on seeded inputs and on the
inputs of the reference's model known-answer tests.  Integer work: every comparison is bit-exact.
"""
import pytest
from exonerate_amd import _abi
import oracle_lib
from golden_util import SETS, SUBOPT_SETS, DERIVED_SETS, SPAN_SETS, ANNOT_SETS, ANNOT_SUBOPT_SETS, load_set, get_model, set_params, expected


@pytest.mark.parametrize("name", sorted(SETS) + sorted(DERIVED_SETS))
def test_oracle_matches_reference_vectors(lib, params, name):
    params = set_params(lib, name)
    model = get_model(lib, params, name)
    recs = load_set(name)
    assert recs
    for rec in recs:
        q, t = rec["query"].encode(), rec["target"].encode()
        assert oracle_lib.find_score(model, params, q, t) == rec["score"], rec["id"]
        got = oracle_lib.find_path(model, params, q, t, dpmemory=rec["dpmemory"], qid=rec["id"])
        if "path_score" not in rec:
            assert got is None
            continue
        assert got == expected(rec), rec["id"]


@pytest.mark.parametrize("name", sorted(ANNOT_SETS))
def test_oracle_matches_reference_vectors_with_annotation(lib, params, name):
    """--annotation (match.c:276-281): a DNA query's positions inside its annotated CDS score MATCH_IMPOSSIBLY_LOW_SCORE in a
    1:1 DNA match; the reference ran these pairs with the annotation attached to the query (rec["cds"])."""
    params = set_params(lib, name)
    model = get_model(lib, params, name)
    recs = load_set(name)
    assert recs and any(r["score"] > 0 for r in recs)
    if "global" not in name and "bestfit" not in name:       # (an end-to-end alignment has no empty answer to fall back to)
        assert any(r["score"] == 0 for r in recs)
    changed = 0
    try:
        for rec in recs:
            q, t = rec["query"].encode(), rec["target"].encode()
            oracle_lib.set_annotation(None)
            plain = oracle_lib.find_score(model, params, q, t)
            oracle_lib.set_annotation(rec["cds"])
            assert oracle_lib.find_score(model, params, q, t) == rec["score"], rec["id"]
            changed += plain != rec["score"]
            got = oracle_lib.find_path(model, params, q, t, dpmemory=rec["dpmemory"], qid=rec["id"])
            if "path_score" not in rec:
                assert got is None
                continue
            assert got == expected(rec), rec["id"]
    finally:
        oracle_lib.set_annotation(None)
    assert changed >= len(recs) // 3          # the annotation is what decides these records


@pytest.mark.parametrize("name", sorted(SUBOPT_SETS))
def test_oracle_suboptimal_loop_matches_reference(lib, params, name):
    """SubOpt blocking (subopt.c, viterbi.c:701-704): the successive alignments of the GAM loop and the
    blocked point set after each, as the reference produced them."""
    params = set_params(lib, name)
    model = get_model(lib, params, name)
    for rec in load_set(name):
        q, t = rec["query"].encode(), rec["target"].encode()
        got = oracle_lib.find_paths_subopt(model, params, q, t, rec["dpmemory"], rec["threshold"], 6
                                           if "global" not in name else 3, qid=rec["id"])
        assert len(got) == len(rec["subopt"]), rec["id"]
        for (d, pts), exp in zip(got, rec["subopt"]):
            assert (d["score"], d["region"], d["ops"], d["vulgar"]) == \
                   (exp["path_score"], exp["region"], exp["ops"], exp["vulgar"]), rec["id"]
            if "points" in exp:
                assert pts == exp["points"], rec["id"]


@pytest.mark.parametrize("name", sorted(ANNOT_SUBOPT_SETS))
def test_oracle_suboptimal_loop_matches_reference_with_annotation(lib, params, name):
    """The GAM loop with the annotation attached to the query: the veto and the SubOpt blocking in the same match cells."""
    params = set_params(lib, name)
    model = get_model(lib, params, name)
    recs = load_set(name)
    assert recs
    changed, total = 0, 0
    try:
        for rec in recs:
            q, t = rec["query"].encode(), rec["target"].encode()
            oracle_lib.set_annotation(None)
            plain = oracle_lib.find_paths_subopt(model, params, q, t, rec["dpmemory"], rec["threshold"], 4, qid=rec["id"])
            oracle_lib.set_annotation(rec["cds"])
            got = oracle_lib.find_paths_subopt(model, params, q, t, rec["dpmemory"], rec["threshold"], 4, qid=rec["id"])
            assert len(got) == len(rec["subopt"]), rec["id"]
            for (d, _), exp in zip(got, rec["subopt"]):
                assert (d["score"], d["region"], d["ops"], d["vulgar"]) == \
                       (exp["path_score"], exp["region"], exp["ops"], exp["vulgar"]), rec["id"]
            changed += [d for d, _ in got] != [d for d, _ in plain]
            total += len(got)
    finally:
        oracle_lib.set_annotation(None)
    assert 3 * changed >= len(recs) and total > len(recs)          # the annotation decides, and the loop went round


def _rle(ops):
    out = []
    for o in ops:
        if out and out[-1][0] == o:
            out[-1][1] += 1
        else:
            out.append([o, 1])
    return out


@pytest.mark.parametrize("name,mtype,qa,match_state,span_state", SPAN_SETS)
def test_oracle_span_seam_matches_reference(lib, params, name, mtype, qa, match_state, span_state):
    """cell_end_func / cell_start_func (viterbi.c:728-741,793-799) on BSDP's span models: the END cells the src
    DP reports, and score and path of the dst DP that starts from them, as the reference produced them."""
    src = _abi.Model(); dst = _abi.Model()
    assert lib.c4gpu_model_get_derived(mtype.encode(), qa, 0, params, match_state, span_state, 4, 0, src, None) == 0
    assert lib.c4gpu_model_get_derived(mtype.encode(), qa, 0, params, span_state, match_state, 0, 4, dst, None) == 0
    for rec in load_set(name):
        q, t = rec["query"].encode(), rec["target"].encode()
        src_score, cells, dst_score, path = oracle_lib.span_pair(src, dst, params, q, t)
        assert src_score == rec["src_score"], rec["id"]
        assert cells == {(c[0], c[1]): c[2:] for c in rec["end_cells"]}, rec["id"]
        assert dst_score == rec["dst_score"], rec["id"]
        if "path_score" in rec:
            assert path["score"] == rec["path_score"]
            assert [path["query_start"], path["target_start"], path["query_end"] - path["query_start"],
                    path["target_end"] - path["target_start"]] == rec["region"], rec["id"]
            assert _rle(path["ops"]) == rec["ops"], rec["id"]


def test_reference_known_answer_tests(lib, params):
    """src/model/affine.test.c:107-110 (-151/18/32/18), est2genome.test.c:63 (157), protein2dna.test.c:34 (134),
    protein2genome.test.c:34 (125)."""
    kat = {"affine_global_protein": -151, "affine_bestfit_protein": 18, "affine_local_protein": 32,
           "affine_overlap_protein": 18}
    for name, score in kat.items():
        rec = [r for r in load_set(name) if r["id"] == "kat_affine"][0]
        assert rec["score"] == score
        model = get_model(lib, params, name)
        assert oracle_lib.find_score(model, params, rec["query"].encode(), rec["target"].encode()) == score
    rec = [r for r in load_set("est2genome") if r["id"] == "kat_est2genome"][0]
    assert rec["score"] == 157
    for name, rid, score in (("protein2dna", "kat_protein2dna", 134), ("protein2genome", "kat_protein2genome", 125)):
        rec = [r for r in load_set(name) if r["id"] == rid][0]
        assert rec["score"] == score == rec["path_score"]
        model = get_model(lib, params, name)
        assert oracle_lib.find_score(model, params, rec["query"].encode(), rec["target"].encode()) == score
    # vulgar printed by affine.test.c for the local model
    rec = [r for r in load_set("affine_local_protein") if r["id"] == "kat_affine"][0]
    assert rec["vulgar"].endswith("32 M 8 8 G 1 0 M 4 4") and rec["region"] == [11, 33, 13, 12]


def test_oracle_splice_arrays_match_reference(lib, params):
    """SplicePredictor_predict_array_int (splice.c:383) per target, all four site types."""
    import ctypes as C
    olib = oracle_lib.load()
    keys = {"ss5_forward": _abi.SS5_FORWARD, "ss3_forward": _abi.SS3_FORWARD,
            "ss3_reverse": _abi.SS3_REVERSE, "ss5_reverse": _abi.SS5_REVERSE}
    for name in ("est2genome", "est2genome_forcegtag"):
        params = set_params(lib, name)
        for rec in load_set(name):
            t = rec["target"].encode()
            for key, k in keys.items():
                out = (C.c_int32 * len(t))()
                olib.oracle_splice_predict(params.splice[k], t, len(t), out)
                assert list(out) == rec[key], (name, rec["id"], key)


def test_memory_decisions(lib, params):
    """Viterbi_use_reduced_space at the default -D 32: 1 kb x 1 kb affine already exceeds it
    (SURVEY.md section 9), a 300 x 300 rectangle does not."""
    olib = oracle_lib.load()
    model = get_model(lib, params, "affine_local_dna")
    assert olib.oracle_use_reduced_space(model, _abi.Region(0, 0, 1000, 1000), 32) == 1
    assert olib.oracle_use_reduced_space(model, _abi.Region(0, 0, 300, 300), 32) == 0
    assert olib.oracle_use_reduced_space(model, _abi.Region(0, 0, 6, 1000), 0) == 0   # <= 6 x max advance
