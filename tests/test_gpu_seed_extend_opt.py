"""c4gpu_seed_extend_opt (Engine.seed_extend with mask_query / mask_target / seed_repeat: the one-call seeder for soft-masked sets
and --seedrepeat > 1) against seed_fused_opt_cases.replay_opt -- pinned in tests/test_seed_fused_opt_cases.py on the existing
yardsticks and on the reference binary's recorded output -- HSP for HSP in walk order, with all four counters: the recorded
soft-masked and --seedrepeat pairs, the generated cases, the edge shapes of the plain call with lower-case stretches planted or a
repeat of 2; that the defaults are c4gpu_seed_extend; both refusals; the capacity protocol under a mask."""
import pytest

import exonerate_amd as ex
import hsp_codon_cases as hc
import seed_fused_cases as sf
import seed_fused_opt_cases as so
from golden_util import load_set
from test_hsp_softmask import SOFTMASK_SETS
from test_seed_chain_sim import GENERATED
from test_seed_fused_opt_cases import REPEAT_SETS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def params():
    return ex.default_params()


def hold(eng, params, c, **over):
    exp, exp_stats = c.replay(params, **over)
    got, stats = c.run(eng, params, **over)
    assert stats == exp_stats, (c.name, over)
    assert got == exp, (c.name, over)
    return got, stats


@pytest.mark.parametrize("name", SOFTMASK_SETS)
def test_recorded_softmasked_pairs(eng, params, name):
    recs = load_set(name)
    par, recs = recs[0]["params"], recs[1:]
    below = 0
    for r in recs:
        got, stats = hold(eng, params, so.record_case(par, r))
        below += stats["n_below"]
        assert {tuple(h) for h in r["masked"]} <= {tuple(h[:4]) for _, _, h in got}      # what the reference binary printed
    assert below >= 6


def test_recorded_softmasked_codon_pairs(eng, params):
    par, recs = hc.load_codon_set("hsp_codon_softmask")
    for r in recs:
        c = so.Case(r["id"], "codon2codon", [r["query"]], r["target"], par["seedlen"], par["dropoff"], par["threshold"],
                    mask_query=r["mask_query"], mask_target=r["mask_target"])
        hold(eng, params, c)


@pytest.mark.parametrize("rep", [1, 2, 3])
@pytest.mark.parametrize("name", REPEAT_SETS)
def test_recorded_seedrepeat_pairs(eng, params, name, rep):
    recs = load_set(name)
    par, recs = recs[0]["params"], recs[1:]
    for r in recs:
        c = so.record_case(par, r, seed_repeat=rep)
        got, _ = hold(eng, params, c)
        assert sorted(h[:4] for _, _, h in got) == r["repeat"][str(rep)], (r["id"], rep)


@pytest.mark.parametrize("name", sorted(GENERATED))
def test_generated_cases(eng, params, name):
    """As tests/test_seed_chain_sim.py drives the host build: the case as it stands, the same scan strings under the plain rule,
    another repeat value, and mask and repeat together."""
    c = GENERATED[name]()
    hold(eng, params, c)
    if c.mask_query or c.mask_target:
        hold(eng, params, c, mask_query=False, mask_target=False)
    if c.match != "protein2dna":
        hold(eng, params, c, seed_repeat=3 if c.seed_repeat == 2 else 2)
        if c.mask_query or c.mask_target:
            hold(eng, params, c, seed_repeat=1)


@pytest.mark.parametrize("name", [s[0] for s in sf.EDGE_SHAPES])
def test_the_defaults_are_the_plain_call(eng, params, name):
    """(False, False, 1) through the keyword route and c4gpu_seed_extend_opt itself: what c4gpu_seed_extend gives."""
    import ctypes as C
    from exonerate_amd import _abi
    c = sf.case_edge(name)
    plain = c.run(eng, params)
    assert plain == eng.seed_extend(params, c.match, c.pairs, c.width, c.wordlen, c.words, c.emits, c.strings, c.tpos_scale,
                                    c.tpos_offset, c.tpos_modifier, c.seedlen, c.dropoff, c.threshold, mask_query=False,
                                    mask_target=False, seed_repeat=1)
    # the new entry point itself with (0, 0, 1)
    arr, keep = ex._pairs(c.pairs)
    tab = ex._wordtab(eng.ctx, c.width, c.wordlen, c.words)
    try:
        ce = (_abi.SeedEmit * len(c.emits))(*[_abi.SeedEmit(p, q) for p, q in c.emits])
        assert _abi.load().c4gpu_wordtab_set_emissions(tab, ce, len(c.emits)) == 0
        strs = [bytes(x) for x in c.strings]
        sp = (C.c_char_p * len(strs))(*strs)
        sn = (C.c_int32 * len(strs))(*[len(x) for x in strs])
        off = (C.c_int32 * len(strs))(*c.tpos_offset)
        room = plain[1]["n_kept"]
        out, stats = (_abi.SeedHsp * max(1, room))(), _abi.SeedExtendStats()
        assert _abi.load().c4gpu_seed_extend_opt(eng.ctx, tab, params, ex._match_kind(c.match), arr, len(c.pairs), sp, sn, len(strs),
                                                 c.tpos_scale, off, c.tpos_modifier, c.seedlen, c.dropoff, c.threshold, 0, 0, 1, out,
                                                 room, C.byref(stats)) == 0
        assert [(out[i].seed, out[i].pair, out[i].hsp.aslist()) for i in range(room)] == plain[0]
        assert dict(n_hits=stats.n_hits, n_extended=stats.n_extended, n_below=stats.n_below, n_kept=stats.n_kept) == plain[1]
    finally:
        _abi.load().c4gpu_wordtab_destroy(tab)


def test_first_hits_serve_the_call(eng, params):
    c = so.case_edge_opt("edge_2048_257")
    first = []
    eng.seed_extend(params, c.match, c.pairs, c.width, c.wordlen, c.words, c.emits, c.strings, c.tpos_scale, c.tpos_offset,
                    c.tpos_modifier, c.seedlen, c.dropoff, c.threshold, first_hits=first, mask_target=True)
    exp = [-1] * len(c.queries)
    for k, (qi, _, _) in enumerate(c.calls):
        if exp[qi] < 0:
            exp[qi] = k
    assert first == exp and max(exp) >= 0


def test_capacity_under_a_mask(eng, params):
    c = so.case_edge_opt("edge_2049_65535")
    exp, exp_stats = c.replay(params)
    assert exp_stats["n_kept"] >= 3
    got, stats = c.run(eng, params, cap=exp_stats["n_kept"] - 1)
    assert got == [] and stats == exp_stats                # nothing written, the counters say how much room is needed
    got, stats = c.run(eng, params, cap=stats["n_kept"])
    assert got == exp and stats == exp_stats


def test_refusals(eng, params):
    """Both refusals, each with its own text, before anything is launched; the context serves a case afterwards."""
    c = so.case_tag()
    with pytest.raises(ex.C4GpuError, match="seed_repeat below 1"):
        c.run(eng, params, seed_repeat=0)
    with pytest.raises(ex.C4GpuError, match="seed_repeat below 1"):
        c.run(eng, params, seed_repeat=-3, mask_target=True)
    p = so.case_one_lower_base("protein2dna")
    with pytest.raises(ex.C4GpuError, match="not served for PROTEIN2DNA"):
        p.run(eng, params, seed_repeat=2)
    with pytest.raises(ex.C4GpuError, match="not served for PROTEIN2DNA"):
        p.run(eng, params, seed_repeat=2, mask_target=False)
    hold(eng, params, p)
    hold(eng, params, c)
