"""The ner model (non-equivalenced regions, src/model/ner.c:66-114) on the host: the builder's closed table, the C ABI around it, and
the CPU oracle run on that table against records of the reference itself (tests/golden/ner_*_open0*.jsonl, made by
oracle/_ref/refdump, whose ner open penalty is 0: tests/ner_cases.py).  The op ids of those records pin the table's transition
order -- at penalty 0 the two loops of the ner state tie everywhere, so every tie-break of the reference shows.  Integer work:
every comparison is exact."""
import ctypes as C

import pytest

import exonerate_amd as ex
from exonerate_amd import _abi
import oracle_lib
from golden_util import expected
from ner_cases import REFDUMP_SETS, SUBOPT_SETS, ANNOT_SETS, NER_OPEN_DEFAULT, SUBOPT_MAX, open0_model, load_set


@pytest.mark.parametrize("qa,ta,match", [(0, 0, "dna2dna"), (1, 1, "protein2protein")])
def test_model_get_ner(lib, params, qa, ta, match):
    m = _abi.Model()
    assert lib.c4gpu_model_get(b"ner", qa, ta, params, m) == 0, "c4gpu_model_get does not know the type 'ner'"
    assert m.name.decode() == "NER:affine:local:" + match
    assert (m.n_states, m.n_transitions, m.n_calcs, m.n_shadows) == (6, 13, 4, 0)
    assert (m.max_query_advance, m.max_target_advance, m.total_shadow_designations) == (1, 1, 0)
    assert (m.start_scope, m.end_scope) == (_abi.SCOPE_ANYWHERE, _abi.SCOPE_ANYWHERE)
    assert [m.state_names[k].value.decode() for k in range(6)] == ["START", "END", "match", "insert", "delete", "ner"]
    calc = {m.calcs[k].name.decode(): m.calcs[k] for k in range(4)}
    assert sorted(calc) == ["gap extend", "gap open", "match", "ner open"]
    no = calc["ner open"]
    assert (no.kind, no.value, no.max_score, no.protect) == (_abi.CALC_CONST, NER_OPEN_DEFAULT, NER_OPEN_DEFAULT, 0)
    tr = {m.transitions[k].name.decode(): m.transitions[k] for k in range(13)}
    ner = 5
    for name, inp, out, aq, at, has_calc, label in (("match to ner", 2, ner, 1, 1, True, _abi.LABEL_NER),
                                                    ("ner to match", ner, 2, 0, 0, False, _abi.LABEL_NONE),
                                                    ("ner loop insert", ner, ner, 1, 0, False, _abi.LABEL_NER),
                                                    ("ner loop delete", ner, ner, 0, 1, False, _abi.LABEL_NER)):
        t = tr[name]
        assert (t.input, t.output, t.advance_query, t.advance_target, t.label) == (inp, out, aq, at, label), name
        assert (t.calc >= 0) == has_calc, name
        if has_calc:
            assert m.calcs[t.calc].name == b"ner open"
    assert lib.c4gpu_model_is_accelerated(m) == 1
    assert lib.c4gpu_model_device_family(m) >= 0
    buf = C.create_string_buffer(256)
    lib.c4gpu_model_plugin_name(m, _abi.MODE_FIND_SCORE, 0, buf, 256)
    # Codegen_clean_path_component("optimal:NER:affine:local:<match> find score"): ':' = 58, ' ' = 32
    assert buf.value.decode() == "optimal_58_NER_58_affine_58_local_58_%s_32_find_32_score" % match


def test_both_alphabets_share_the_device_family(lib, params):
    fam = {}
    for kind in ("affine:local", "ner"):
        for a in (0, 1):
            m = _abi.Model()
            assert lib.c4gpu_model_get(kind.encode(), a, a, params, m) == 0
            fam[kind, a] = lib.c4gpu_model_device_family(m)
    assert fam["affine:local", 0] == fam["affine:local", 1] >= 0       # the scoring matrix is a run-time parameter
    assert fam["ner", 0] == fam["ner", 1] >= 0
    assert fam["ner", 0] != fam["affine:local", 0]


@pytest.mark.parametrize("value", [0, -20, -35, -300000000, 7])
def test_model_get_ner_takes_the_open_penalty(lib, params, value):
    m = _abi.Model()
    assert lib.c4gpu_model_get_ner(0, 0, params, value, m) == 0
    calc = [m.calcs[k] for k in range(m.n_calcs) if m.calcs[k].name == b"ner open"]
    assert len(calc) == 1 and (calc[0].value, calc[0].max_score) == (value, value)
    d = _abi.Model()
    assert lib.c4gpu_model_get(b"ner", 0, 0, params, d) == 0
    assert lib.c4gpu_model_device_family(m) == lib.c4gpu_model_device_family(d)      # the penalty is a run-time value too
    py = ex.Model("ner", ner_open=value)
    assert bytes(py.c) == bytes(m)
    assert bytes(ex.Model("ner").c) == bytes(d)
    with pytest.raises(ex.C4GpuError):
        ex.Model("affine:local", ner_open=value)


def test_ner_has_no_mixed_alphabet_form(lib, params):
    m = _abi.Model()
    assert lib.c4gpu_model_get(b"ner", 0, 1, params, m) != 0                        # dna2protein: not accelerated
    assert lib.c4gpu_model_get_ner(0, 1, params, -20, m) != 0


@pytest.mark.parametrize("name", sorted(REFDUMP_SETS))
def test_oracle_on_the_ner_table_matches_reference_vectors(name):
    model = open0_model(name)
    recs = load_set(name)
    assert recs
    labels = set()
    for rec in recs:
        q, t = rec["query"].encode(), rec["target"].encode()
        assert rec["model"] == model.name
        assert oracle_lib.find_score(model.c, model.params, q, t) == rec["score"], rec["id"]
        got = oracle_lib.find_path(model.c, model.params, q, t, dpmemory=rec["dpmemory"], qid=rec["id"])
        assert got == expected(rec), rec["id"]
        labels |= {model.c.transitions[o[0]].label for o in rec["ops"]}
    assert _abi.LABEL_NER in labels and _abi.LABEL_MATCH in labels
    if name == "ner_dna_open0":
        # both loops of the ner state and long queries (several strips of query rows on the device) are in the set
        names = {model.c.transitions[o[0]].name.decode() for rec in recs for o in rec["ops"]}
        assert {"match to ner", "ner loop insert", "ner loop delete", "ner to match"} <= names
        assert sum(300 <= rec["qlen"] <= 1200 for rec in recs) >= 3 and max(rec["qlen"] for rec in recs) > 512


@pytest.mark.parametrize("name", sorted(ANNOT_SETS))
def test_oracle_on_the_ner_table_matches_reference_vectors_with_annotation(name):
    """--annotation (match.c:276-281): the ner model's DNA form scores its matches with the same 1:1 DNA match function, so a
    query position inside the annotated CDS (rec["cds"]) can only sit in a gap or in a non-equivalenced region."""
    model = open0_model(name)
    recs = load_set(name)
    assert recs
    changed = 0
    try:
        for rec in recs:
            q, t = rec["query"].encode(), rec["target"].encode()
            assert rec["model"] == model.name
            oracle_lib.set_annotation(None)
            plain = oracle_lib.find_path(model.c, model.params, q, t, dpmemory=rec["dpmemory"], qid=rec["id"])
            oracle_lib.set_annotation(rec["cds"])
            assert oracle_lib.find_score(model.c, model.params, q, t) == rec["score"], rec["id"]
            got = oracle_lib.find_path(model.c, model.params, q, t, dpmemory=rec["dpmemory"], qid=rec["id"])
            assert got == (expected(rec) if "path_score" in rec else None), rec["id"]
            changed += got != plain
    finally:
        oracle_lib.set_annotation(None)
    assert 3 * changed >= len(recs)           # the annotation is what decides these records


@pytest.mark.parametrize("name", sorted(SUBOPT_SETS))
def test_oracle_suboptimal_loop_on_the_ner_table_matches_reference(name):
    model = open0_model(name)
    total = 0
    for rec in load_set(name):
        q, t = rec["query"].encode(), rec["target"].encode()
        got = oracle_lib.find_paths_subopt(model.c, model.params, q, t, rec["dpmemory"], rec["threshold"], SUBOPT_MAX, qid=rec["id"])
        assert len(got) == len(rec["subopt"]), rec["id"]
        for (d, pts), exp in zip(got, rec["subopt"]):
            assert (d["score"], d["region"], d["ops"], d["vulgar"]) == \
                   (exp["path_score"], exp["region"], exp["ops"], exp["vulgar"]), rec["id"]
            if "points" in exp:
                assert pts == exp["points"], rec["id"]
        total += len(got)
    assert total > 2 * len(load_set(name))               # the loop really went round
