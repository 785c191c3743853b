"""hsp_entry_step (exonerate_amd/csrc/c4_hsp_extend.h) -- the step seed_chain_kernel takes seed by seed on one horizon entry --
compiled for the host (tests/seed_chain_sim.hip) and driven over walks grouped by entry, against replay_opt
(tests/seed_fused_opt_cases.py) on everything tests/test_seed_fused_opt_cases.py pins that yardstick on: the seeder records with
the options off, the recorded soft-masked pairs, the recorded --seedrepeat pairs at 1, 2 and 3, and every generated case.  The
very code the kernel runs, without a GPU."""
import pytest

import exonerate_amd as ex
import hsp_codon_cases as hc
import seed_chain_sim_lib as sim
import seed_fused_cases as sf
import seed_fused_opt_cases as so
from golden_util import load_set
from test_hsp_softmask import SOFTMASK_SETS
from test_oracle_seed import load_seed_set
from test_seed_fused_opt_cases import RECORDS, REPEAT_SETS


@pytest.fixture(scope="module")
def params():
    return ex.default_params()


def check(params, match, queries, target, calls, seedlen, dropoff, threshold, **opt):
    detail = {}
    exp = so.replay_opt(params, match, queries, target, calls, seedlen, dropoff, threshold, detail=detail, **opt)
    kept, stats, verdict = sim.walk(params, match, queries, target, calls, seedlen, dropoff, threshold, **opt)
    assert verdict == detail["verdict"]
    assert (kept, stats) == exp
    return stats, detail


def check_case(params, c, **over):
    opt = dict(mask_query=c.mask_query, mask_target=c.mask_target, seed_repeat=c.seed_repeat)
    opt.update(over)
    return check(params, c.match, c.queries, c.target, c.calls, c.seedlen, c.dropoff, c.threshold, **opt)


@pytest.mark.parametrize("point", ["default", "low"])
@pytest.mark.parametrize("name,k", RECORDS)
def test_seeder_records_with_the_options_off(params, name, k, point):
    rec = load_seed_set(name)[k]
    dropoff, threshold = sf.points(rec["match"])[point]
    stats, _ = check(params, rec["match"], rec["queries"], rec["target"], rec["expected"], rec["wordlen"], dropoff, threshold)
    assert 0 < stats["n_extended"] < stats["n_hits"]


@pytest.mark.parametrize("name", SOFTMASK_SETS)
def test_recorded_softmasked_pairs(params, name):
    recs = load_set(name)
    par, recs = recs[0]["params"], recs[1:]
    n_dropped = 0
    for r in recs:
        for masked in (False, True):
            c = so.record_case(par, r, masked=masked)
            n_dropped += len(check_case(params, c)[1]["dropped"])
    assert n_dropped >= 6


def test_recorded_softmasked_codon_pairs(params):
    par, recs = hc.load_codon_set("hsp_codon_softmask")
    for r in recs:
        check(params, "codon2codon", [r["query"]], r["target"], [[0, qs, ts] for qs, ts in r["seeds"]], par["seedlen"],
              par["dropoff"], par["threshold"], mask_query=r["mask_query"], mask_target=r["mask_target"])


@pytest.mark.parametrize("rep", [1, 2, 3])
@pytest.mark.parametrize("name", REPEAT_SETS)
def test_recorded_seedrepeat_pairs(params, name, rep):
    recs = load_set(name)
    par, recs = recs[0]["params"], recs[1:]
    for r in recs:
        check_case(params, so.record_case(par, r, seed_repeat=rep))


GENERATED = {"dropped_then_extended": so.case_dropped_then_extended, "masked_keeps_fewer": so.case_masked_keeps_fewer,
             "tag": so.case_tag, "codon_wrapped_shared_entry": so.case_codon_wrapped_shared_entry,
             "mask_at_the_ends": so.case_mask_at_the_ends,
             "one_lower_base_protein2dna": lambda: so.case_one_lower_base("protein2dna"),
             "one_lower_base_codon2codon": lambda: so.case_one_lower_base("codon2codon")}
for _m in ("dna2dna", "protein2protein"):
    for _r in (2, 3):
        GENERATED["counters_%s_%d" % (_m, _r)] = lambda m=_m, r=_r: so.case_counters(m, r)
for _s in sf.EDGE_SHAPES:
    GENERATED[_s[0] + "_masked"] = lambda n=_s[0]: so.case_edge_opt(n)
    GENERATED[_s[0] + "_repeat2"] = lambda n=_s[0]: so.case_edge_opt(n, seed_repeat=2)


@pytest.mark.parametrize("name", sorted(GENERATED))
def test_generated_cases(params, name):
    c = GENERATED[name]()
    check_case(params, c)
    if c.mask_query or c.mask_target:
        check_case(params, c, mask_query=False, mask_target=False)         # the same scan strings under the plain rule
    if c.match != "protein2dna":
        check_case(params, c, seed_repeat=3 if c.seed_repeat == 2 else 2)
        if c.mask_query or c.mask_target:
            check_case(params, c, seed_repeat=1)
