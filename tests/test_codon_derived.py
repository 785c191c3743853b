"""BSDP's derived models of coding2coding without a device: the host builder's three tables and the CPU oracle against the
reference's records (tests/golden/derived_coding2coding*.jsonl, tools/make_codon_derived_golden.py), the device families the
tables resolve to, and the heuristic seam of the drop-in in its host mode (C4GPU_BSDP_HOST=1: the seam's collecting, dry runs and
replay around the reference's own DPs), byte for byte against the unmodified reference.  The device itself:
tests/test_gpu_codon_derived.py."""
import pytest

import exonerate_amd as ex
from exonerate_amd import _abi
import codon_cases as cc
import codon_derived_cases as cd

needs_binaries = pytest.mark.skipif(not cd.HAVE_BINARIES, reason="reference binaries are built in the build container (make -C integration)")


@pytest.mark.parametrize("name", cd.SETS)
def test_builder_tables_replay_the_reference_records(name):
    """Every recorded operation list walks the builder's derived table from START to END and adds up to the recorded score over the
    recorded region; the model is named as the reference names it."""
    model = cd.set_model(name)
    assert model.c.max_query_advance == 3 and model.c.n_states == 7
    assert model.c.n_transitions == (29 if cd.set_role(name) == "join" else 23)
    recs = cd.records(name)
    assert 0 < len(recs) <= 40
    paths = 0
    for rec in recs:
        assert rec["model"] == cd.REF_NAME[cd.set_role(name)] == model.c.name.decode(), rec["id"]
        if "path_score" not in rec:
            continue
        paths += 1
        score, dq, dt, _ = cc.replay(model, rec)
        assert (score, dq, dt) == (rec["path_score"], rec["region"][2], rec["region"][3]), rec["id"]
        assert rec["path_score"] == rec["score"], rec["id"]
    assert paths >= len(recs) * 3 // 4


@pytest.mark.parametrize("name", cd.SETS)
def test_oracle_equals_every_record(name):
    model = cd.set_model(name)
    for rec in cd.records(name):
        q, t = rec["query"], rec["target"]
        whole = (0, 0, len(q), len(t))
        score, region, ops = cd.expected(rec)
        assert cd.oracle(model, ex.MODE_FIND_SCORE, q, t, whole)[0] == score, rec["id"]
        if ops is not None:
            assert cd.oracle(model, ex.MODE_FIND_PATH, q, t, whole) == (score, region, ops), rec["id"]


def test_fixture_sets_cover_what_the_kernels_can_get_wrong():
    """What tools/make_codon_derived_golden.py asserted when it wrote the sets, restated on the committed files."""
    strip = 64 * cd.ROWS_PER_LANE
    for name in cd.SETS:
        recs = cd.records(name)
        ql, tl = {len(r["query"]) for r in recs}, {len(r["target"]) for r in recs}
        assert {1, 2} <= ql and {1, 2} <= tl, name
        assert strip in ql and strip - 2 in ql, name                    # Q + 1 rows: one more and one fewer than a strip
        assert max(ql) <= 210 and max(tl) <= 60
        small = sum(1 for r in recs if len(r["query"]) <= 49 and len(r["target"]) <= 49)
        assert 4 * small >= 3 * len(recs), name
        if cd.set_role(name) == "join":
            assert {(len(r["query"]) % 3, len(r["target"]) % 3) for r in recs} == {(a, b) for a in range(3) for b in range(3)}


def test_device_families():
    """The three derived tables resolve to compiled device families (and are accelerated); ungapped:trans's derived tables have
    none, so its heuristic runs keep the reference's route."""
    lib = _abi.load()
    fams = set()
    for role, spec in cd.ROLES.items():
        m = ex.Model.derived("coding2coding", *spec)
        assert lib.c4gpu_model_is_accelerated(m.c) == 1
        fam = lib.c4gpu_model_device_family(m.c)
        assert fam >= 0, role
        fams.add(fam)
        assert lib.c4gpu_model_device_family(ex.Model.derived("ungapped:trans", *spec).c) < 0, role
    whole = lib.c4gpu_model_device_family(ex.Model("coding2coding").c)
    assert len(fams) == 3 and whole not in fams and min(fams) > whole          # appended after the whole model: no number moved


# ---- the drop-in, host mode --------------------------------------------------------------------------------------------
@needs_binaries
@pytest.mark.parametrize("extra", [[], ["-S", "no"], ["--refine", "region"], ["--refine", "full", "--bestn", "1"]],
                         ids=["default", "S_no", "refine_region", "refine_full_bestn1"])
def test_heuristic_coding2coding_is_collected_and_byte_identical(tmp_path, extra):
    ref, gpu, err = cd.run_pair(tmp_path, "coding2coding", extra, {"C4GPU_BSDP_HOST": "1"})
    assert gpu == ref
    vulgar = [l for l in ref.decode().splitlines() if l.startswith("vulgar:")]
    if "--bestn" not in extra:
        assert sum(" F " in l for l in vulgar) >= 4 and sum(" G " in l for l in vulgar) >= 4, vulgar
    assert "has no device family" not in err, err[-1500:]
    got = cd.served(err)
    assert got, err[-1500:]                                  # (absent where the run was not collected)
    s_ok, s_all, p_ok, p_all = got
    assert s_ok > 0 and p_ok > 0, err[-600:]
    if "-S" in extra:                                        # no sub-optimal rounds: nothing is ever blocked, every call is served
        assert (s_ok, p_ok) == (s_all, p_all), err[-600:]
    if "--refine" in extra:
        r = cd.refinements(err)
        assert r and r[0] > 0, err[-800:]                    # the first refinements came from a refinement batch


@needs_binaries
def test_heuristic_ungapped_trans_keeps_the_reference_route(tmp_path):
    ref, gpu, err = cd.run_pair(tmp_path, "ungapped:trans", [], {"C4GPU_BSDP_HOST": "1"})
    assert gpu == ref and ref.count(b"vulgar:") >= 4
    assert "c4gpu bsdp:" not in err, err[-800:]              # not collected: no report line, no warning


@needs_binaries
def test_switching_the_seam_off(tmp_path):
    ref, gpu, err = cd.run_pair(tmp_path, "coding2coding", [], {"C4GPU_BSDP_OFF": "1", "C4GPU_HSP_OFF": "1"})
    assert gpu == ref and "c4gpu bsdp" not in err
