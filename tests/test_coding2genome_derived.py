"""BSDP's derived models of coding2genome without a device: the nine tables of the host builder (terminals and join of match
state 2, span src / dst of the three intron phases) against the reference's records (tests/golden/derived_coding2genome*.jsonl,
span_coding2genome_phase*.jsonl: tools/make_coding2genome_derived_golden.py), the device families they resolve to, what the sets
cover, and the heuristic seam of the drop-in in its host mode (C4GPU_BSDP_HOST=1 C4GPU_CODING2GENOME_BSDP=1: the seam's
collecting, dry runs and replay around the reference's own DPs), byte for byte against the recorded output of the unmodified
reference.  No test routes these models through the CPU oracle (its split-codon calc is the protein query's).  The device itself:
tests/test_gpu_coding2genome_derived.py."""
import pytest

import exonerate_amd as ex
from exonerate_amd import _abi
import coding2genome_cases as cg
import coding2genome_derived_cases as cd

needs_binaries = pytest.mark.skipif(not cd.HAVE_BINARIES, reason="reference binaries are built in the build container (make -C integration)")
HOST = {"C4GPU_BSDP_HOST": "1"}
SWITCH = {"C4GPU_CODING2GENOME_BSDP": "1"}


def test_device_families():
    """Each of the nine derived tables resolves to its own compiled device family, numbered after the whole model's: the families
    were appended and no earlier number moved.  (Before the families existed these calls returned -1.)"""
    lib = _abi.load()
    whole = lib.c4gpu_model_device_family(ex.Model("coding2genome").c)
    fams = {}
    for name, m in cd.all_models().items():
        assert lib.c4gpu_model_is_accelerated(m.c) == 1, name
        fams[name] = lib.c4gpu_model_device_family(m.c)
        assert fams[name] > whole >= 0, (name, fams[name])
    assert len(set(fams.values())) == 9, fams
    # the src traceback model (CORNER / CORNER) runs on the src tables
    for ph in range(3):
        assert lib.c4gpu_model_device_family(cd.span_src(ph, traceback=True).c) == fams["phase%d_span_src" % ph]
    # no earlier family's number has moved: the whole models and a sample of the derived ones, as they were numbered before
    before = [("ungapped", None, 0), ("affine:local", None, 1), ("est2genome", None, 2), ("ner", None, 31), ("ungapped:trans", None, 32),
              ("coding2coding", None, 33), ("coding2coding", (0, 2, 0, 4), 34), ("coding2coding", (2, 2, 4, 4), 36),
              ("coding2genome", None, 37), ("est2genome", (2, 8, 4, 0), 21), ("affine:local", (0, 2, 0, 4), 6)]
    for mtype, spec, fam in before:
        m = ex.Model(mtype) if spec is None else ex.Model.derived(mtype, *spec)
        assert lib.c4gpu_model_device_family(m.c) == fam, (mtype, spec)
    # coding2coding's derived tables are not coding2genome's
    assert lib.c4gpu_model_device_family(ex.Model.derived("coding2coding", 2, 2, 4, 4).c) not in fams.values()


def test_derived_tables():
    """What C4_DerivedModel_create keeps of coding2genome (c4.c:2217-2337): every state stays reachable in all nine models, START
    and END are states 0 and 1, the widest query advance stays 3, the three intron shadows stay, and the scopes are the role's."""
    whole = ex.Model("coding2genome").c
    for name, m in cd.all_models().items():
        c = m.c
        assert (c.n_states, c.start_state, c.end_state) == (14, 0, 1), name
        assert (c.max_query_advance, c.max_target_advance) == (3, 3), name
        assert (c.n_shadows, c.total_shadow_designations, c.n_calcs) == (whole.n_shadows, 1, whole.n_calcs) == (3, 1, 8), name
        assert c.n_transitions == {"start": 39, "end": 39, "join": 48}.get(name, 40), name
        out_of_start = [c.transitions[k] for k in range(c.n_transitions) if c.transitions[k].input == 0]
        if name.endswith("span_dst"):
            # START is the span (intron) state: the intron loop and the 3' splice site, neither advances the query
            assert sorted((t.advance_query, t.advance_target) for t in out_of_start) == [(0, 1), (0, 2)], name
        elif name != "start":
            # START is the match state: query advances of 1, 2 and 3, the 5' site and the split-codon pre transitions
            assert {t.advance_query for t in out_of_start} == {0, 1, 2, 3}, name
            assert {(1, 1), (2, 2), (0, 2), (3, 3)} <= {(t.advance_query, t.advance_target) for t in out_of_start}, name
    scopes = {"start": (0, 4), "end": (4, 0), "join": (4, 4)}
    for role, (ss, es) in scopes.items():
        c = cd.all_models()[role].c
        assert (c.start_scope, c.end_scope) == (ss, es) and c.name.decode() == cd.REF_NAME[role]


@pytest.mark.parametrize("name", cd.SETS)
def test_builder_tables_replay_the_reference_records(name):
    """Every recorded operation list walks the builder's derived table from START to END and adds up -- codon matches, split
    codons across the intron, the recorded splice values -- to the recorded score over the recorded region."""
    model = cd.set_model(name)
    recs = cd.records(name)
    paths = 0
    for rec in recs:
        assert rec["model"] == cd.REF_NAME[cd.set_role(name)] == model.c.name.decode(), rec["id"]
        if "path_score" not in rec:
            continue
        paths += 1
        score, dq, dt, _ = cg.replay(model, rec)
        assert (score, dq, dt) == (rec["path_score"], rec["region"][2], rec["region"][3]), rec["id"]
        assert rec["path_score"] == rec["score"], rec["id"]
    assert paths >= len(recs) * 3 // 4


@pytest.mark.parametrize("phase", range(3))
def test_span_records_walk_the_dst_table(phase):
    dst = cd.span_dst(phase)
    for rec in cd.records(cd.SPAN_SETS[phase]):
        assert cd.walk(dst, rec) == (rec["region"][2], rec["region"][3]), rec["id"]
        assert rec["cell_size"] == 1 + dst.c.total_shadow_designations
        assert rec["path_score"] == rec["dst_score"], rec["id"]
        # the dst path starts in one of the src DP's END cells
        assert (rec["region"][0], rec["region"][1]) in {(c[0], c[1]) for c in rec["end_cells"]}, rec["id"]


def test_fixture_sets_cover_what_the_kernels_can_get_wrong():
    """What tools/make_coding2genome_derived_golden.py asserted when it wrote the sets, restated on the committed files: the test
    fails if a set is regenerated poorer."""
    for name in cd.SETS:
        cd.check_set(cd.set_model(name), [dict(r) for r in cd.records(name)], cd.set_role(name))
    for phase in range(3):
        cd.check_span_set(cd.span_dst(phase), list(cd.records(cd.SPAN_SETS[phase])), phase)
    cd.check_cli(cd.load_cli())


def test_the_alt_point_moves_what_it_says():
    d, a = ex.default_params(), cd.set_params("derived_coding2genome_alt_join")
    for field in ("codon_gap_open", "codon_gap_extend", "frameshift_penalty", "intron_open_penalty", "min_intron", "max_intron"):
        assert getattr(d, field) != getattr(a, field), field


# ---- the drop-in, host mode --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    data = cd.load_cli()
    assert (data["queries"], data["targets"]) == tuple([list(x) for x in side] for side in cd.cli_inputs())
    return data


@needs_binaries
@pytest.mark.parametrize("variant", sorted(cd.CLI_VARIANTS))
def test_heuristic_coding2genome_is_collected_and_byte_identical(tmp_path, cli, variant):
    extra = cd.CLI_REPORTS + cd.CLI_VARIANTS[variant]
    _, gpu, err = cd.run_pair(tmp_path, "coding2genome", extra, dict(HOST, **SWITCH), inputs=cd.cli_inputs(), ref=False)
    assert cd.stable_lines(gpu) == cd.cli_stdout(cli, variant)
    assert "has no device family" not in err, err[-1500:]
    got = cd.served(err)
    assert got, err[-1500:]
    s_ok, s_all, p_ok, p_all = got
    assert s_ok > 0 and p_ok > 0, err[-600:]
    spans = int(err.split(" spans) in device batches")[0].rsplit("(", 1)[1])
    assert spans > 0, err[-600:]
    if variant == "S_no":                                    # no sub-optimal rounds: nothing is ever blocked, every call is served
        assert (s_ok, p_ok) == (s_all, p_all), err[-600:]
    if variant == "default":                                 # the share the device test's floor (0.7 of calls) is held against
        assert s_ok + p_ok >= 0.7 * (s_all + p_all), err[-600:]
    if variant.startswith("refine"):
        r = cd.refinements(err)
        assert r and r[0] > 0, err[-800:]


@needs_binaries
def test_without_the_switch_the_run_is_the_references(tmp_path, cli):
    """C4GPU_CODING2GENOME and C4GPU_CODING2GENOME_SDP are other seams' switches: with them, as with nothing set, a heuristic
    --gappedextension no run of coding2genome stays with the reference, and says so."""
    for env in (HOST, dict(HOST, C4GPU_CODING2GENOME="1", C4GPU_CODING2GENOME_SDP="1")):
        _, gpu, err = cd.run_pair(tmp_path, "coding2genome", cd.CLI_REPORTS, env, inputs=cd.cli_inputs(), ref=False)
        assert cd.stable_lines(gpu) == cd.cli_stdout(cli, "default")
        assert "stays with the reference" in err and cd.served(err) is None, err[-1500:]
