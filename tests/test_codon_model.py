"""The translated models on the host: ungapped:trans (src/model/ungapped.c:106-166 with Match_Type_CODON2CODON) and coding2coding
(src/model/coding2coding.c:50-66 = Affine_create(LOCAL, DNA, DNA, translate_both) + Frameshift_add on the query and on the target,
src/model/frameshift.c:75-125).  The builder's closed tables against the reference's construction, written out literally here
(refdump's table dump does not know these two models); the transition ids -- the evaluation and tie-break order -- are anchored by
replaying the op ids of the reference's own paths (tests/golden/coding2coding*.jsonl, ungapped_trans*.jsonl) through the tables:
they must chain from START to END, advance exactly over the recorded region and add up to the recorded score.  Integer work: every
comparison is exact."""
import ctypes as C

import pytest

import exonerate_amd as ex
from exonerate_amd import _abi
from codon_cases import REFDUMP_SETS, SUBOPT_SETS, MODEL_NAME, set_model, load_set, replay

G, F, M, N = _abi.LABEL_GAP, _abi.LABEL_FRAMESHIFT, _abi.LABEL_MATCH, _abi.LABEL_NONE
# name -> (input, output, advance_query, advance_target, calc name or None, label); states: 0 START, 1 END, then in creation order
UNGAPPED = {"states": ["START", "END", "match"],
            "calcs": ["match"],
            "transitions": {"start to match": (0, 2, 0, 0, None, N), "match to end": (2, 1, 0, 0, None, N),
                            "match": (2, 2, 3, 3, "match", M)}}
CODING = {"states": ["START", "END", "match", "insert", "delete", "frameshift query", "frameshift target"],
          "calcs": ["match", "gap open", "gap extend", "frameshift"],
          "transitions": {
              "start to match": (0, 2, 0, 0, None, N), "match to end": (2, 1, 0, 0, None, N), "match": (2, 2, 3, 3, "match", M),
              "match to insert": (2, 3, 3, 0, "gap open", G), "match to delete": (2, 4, 0, 3, "gap open", G),
              "insert": (3, 3, 3, 0, "gap extend", G), "insert to match": (3, 2, 0, 0, None, N),
              "delete": (4, 4, 0, 3, "gap extend", G), "delete to match": (4, 2, 0, 0, None, N),
              "frameshift open 1 query": (2, 5, 1, 0, "frameshift", F), "frameshift open 2 query": (2, 5, 2, 0, "frameshift", F),
              "frameshift close 0 query": (5, 2, 0, 0, None, N), "frameshift close 3 query": (5, 2, 3, 0, None, F),
              "frameshift open 1 target": (2, 6, 0, 1, "frameshift", F), "frameshift open 2 target": (2, 6, 0, 2, "frameshift", F),
              "frameshift close 0 target": (6, 2, 0, 0, None, N), "frameshift close 3 target": (6, 2, 0, 3, None, F)}}


@pytest.mark.parametrize("kind,table", [("ungapped:trans", UNGAPPED), ("coding2coding", CODING)])
def test_model_get_builds_the_reference_s_table(lib, params, kind, table):
    m = _abi.Model()
    assert lib.c4gpu_model_get(kind.encode(), 0, 0, params, m) == 0, "c4gpu_model_get does not know the type %r" % kind
    assert m.name.decode() == MODEL_NAME[kind]
    ns, nt, nc = len(table["states"]), len(table["transitions"]), len(table["calcs"])
    assert (m.n_states, m.n_transitions, m.n_calcs, m.n_shadows) == (ns, nt, nc, 0)
    assert (ns, nt, nc) == ((3, 3, 1) if kind == "ungapped:trans" else (7, 17, 4))
    assert (m.max_query_advance, m.max_target_advance, m.total_shadow_designations) == (3, 3, 0)
    assert (m.start_scope, m.end_scope) == (_abi.SCOPE_ANYWHERE, _abi.SCOPE_ANYWHERE)
    assert (m.query_alphabet, m.target_alphabet) == (0, 0)
    assert [m.state_names[k].value.decode() for k in range(ns)] == table["states"]
    assert [m.calcs[k].name.decode() for k in range(nc)] == table["calcs"]
    tr = {m.transitions[k].name.decode(): m.transitions[k] for k in range(nt)}
    assert sorted(tr) == sorted(table["transitions"])
    for name, (inp, out, aq, at, calc, label) in table["transitions"].items():
        t = tr[name]
        assert (t.input, t.output, t.advance_query, t.advance_target, t.label) == (inp, out, aq, at, label), name
        assert (m.calcs[t.calc].name.decode() if t.calc >= 0 else None) == calc, name
        assert t.dst_shadow_mask == 0
    calc = {m.calcs[k].name.decode(): m.calcs[k] for k in range(nc)}
    mx = max(params.protein_submat[i][j] for i in range(24) for j in range(24))
    assert (calc["match"].kind, calc["match"].max_score, calc["match"].protect) == (_abi.CALC_MATCH_CODON, mx, 0)
    if kind == "coding2coding":
        # a match of advance 3 makes Affine's calcs return the codon penalties (affine.c:88-124); their bound stays the plain one
        assert (calc["gap open"].kind, calc["gap open"].value, calc["gap open"].max_score) == (_abi.CALC_CONST, params.codon_gap_open, params.gap_open)
        assert (calc["gap extend"].kind, calc["gap extend"].value, calc["gap extend"].max_score) == (_abi.CALC_CONST, params.codon_gap_extend, params.gap_extend)
        assert (calc["frameshift"].kind, calc["frameshift"].value, calc["frameshift"].max_score) == \
               (_abi.CALC_CONST, params.frameshift_penalty, params.frameshift_penalty)
    assert lib.c4gpu_model_is_accelerated(m) == 1
    assert lib.c4gpu_model_device_family(m) >= 0
    buf = C.create_string_buffer(256)
    lib.c4gpu_model_plugin_name(m, _abi.MODE_FIND_SCORE, 0, buf, 256)
    assert buf.value.decode().startswith("optimal_58_" + MODEL_NAME[kind].replace(":", "_58_") + "_32_find_32_score")


def test_the_two_models_have_device_families_of_their_own(lib, params):
    fam = {}
    for kind in ("affine:local", "ungapped", "ungapped:trans", "coding2coding"):
        m = _abi.Model()
        assert lib.c4gpu_model_get(kind.encode(), 0, 0, params, m) == 0, kind
        fam[kind] = lib.c4gpu_model_device_family(m)
    assert len(set(fam.values())) == 4 and min(fam.values()) >= 0, fam


def test_translated_models_take_dna_only(lib, params):
    m = _abi.Model()
    for kind in (b"ungapped:trans", b"coding2coding"):
        for qa, ta in ((1, 1), (1, 0), (0, 1), (2, 2)):
            assert lib.c4gpu_model_get(kind, qa, ta, params, m) != 0
    assert lib.c4gpu_model_get(b"affine:local", 2, 2, params, m) != 0          # the codon form is not a caller's alphabet
    with pytest.raises(ex.C4GpuError):
        ex.Model("coding2coding", query_alphabet=1)
    assert bytes(ex.Model("coding2coding").c) == bytes(ex.Model("coding2coding", query_alphabet=0, target_alphabet=0).c)


def test_abi_binds_the_additions(lib, params):
    assert _abi.CALC_MATCH_CODON == 8 and _abi.CALC_PHASE_POST == 7                # appended: no number moved
    h = lib.c4m_coding2coding_create(params)
    assert h
    m, d = _abi.Model(), _abi.Model()
    assert lib.c4m_flatten(h, m) == 0
    lib.c4m_model_destroy(h)
    assert lib.c4gpu_model_get(b"coding2coding", 0, 0, params, d) == 0
    assert bytes(m) == bytes(d)
    assert lib.c4gpu_abi_version() == _abi.ABI_VERSION == 9


def test_penalties_follow_the_parameters(lib):
    model = set_model("coding2coding_codonalt")
    calc = {model.c.calcs[k].name.decode(): model.c.calcs[k].value for k in range(model.c.n_calcs)}
    assert (calc["gap open"], calc["gap extend"], calc["frameshift"]) == (-11, -3, -13)
    d = ex.Model("coding2coding")
    assert lib.c4gpu_model_device_family(model.c) == lib.c4gpu_model_device_family(d.c)      # run-time values


@pytest.mark.parametrize("name", sorted(REFDUMP_SETS))
def test_golden_ops_replay_to_the_recorded_region_and_score(name):
    model = set_model(name)
    recs = load_set(name)
    assert recs
    labels, used = set(), set()
    for rec in recs:
        assert rec["model"] == model.c.name.decode()
        assert rec["ops"], rec["id"]                                              # every record carries a path
        score, dq, dt, seen = replay(model, rec)
        assert (dq, dt) == tuple(rec["region"][2:]), rec["id"]
        assert score == rec["path_score"] == rec["score"], rec["id"]
        labels |= seen
        used |= {o[0] for o in rec["ops"]}
    if REFDUMP_SETS[name] == "coding2coding":
        assert {M, G, F} <= labels
        if name == "coding2coding":
            assert used == set(range(model.c.n_transitions)) - {0} or used == set(range(model.c.n_transitions)), sorted(used)
            names = {model.c.transitions[k].name.decode() for k in used}
            assert {"frameshift open 1 query", "frameshift open 2 query", "frameshift close 3 query", "frameshift open 1 target",
                    "frameshift open 2 target", "match to insert", "insert", "match to delete", "delete"} <= names
            # the shapes the device kernels care about
            ql = sorted(r["qlen"] for r in recs)
            assert ql[:5] == [1, 2, 3, 4, 5] and 18 in ql and 19 in ql and ql[-1] >= 640 and 384 <= ql[-2] < 640
            assert any(r["region"][0] % 3 and r["region"][1] % 3 for r in recs)      # regions that start off frame
    else:
        assert labels == {M, N} and used == {0, 1, 2}


@pytest.mark.parametrize("name", sorted(SUBOPT_SETS))
def test_suboptimal_records_replay_too(name):
    model = set_model(name)
    total = 0
    for rec in load_set(name):
        assert rec["subopt"], rec["id"]
        for a in rec["subopt"]:
            r = dict(rec, ops=a["ops"], region=a["region"])
            score, dq, dt, _ = replay(model, r)
            assert (score, dq, dt) == (a["path_score"], a["region"][2], a["region"][3]), rec["id"]
        scores = [a["path_score"] for a in rec["subopt"]]
        assert scores == sorted(scores, reverse=True) and scores[-1] >= rec["threshold"]
        total += len(rec["subopt"])
    assert total > len(load_set(name))                                            # the loop really went round
