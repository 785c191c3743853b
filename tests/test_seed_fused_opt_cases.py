"""The yardstick of c4gpu_seed_extend_opt pinned before anything is held to it (CPU): seed_fused_opt_cases.replay_opt
(a) with masks off and repeat 1 equals seed_fused_cases.replay on every reference-generated seeder record at both dropoff /
    threshold points;
(b) with masks on equals test_hsp_softmask.seed_set -- and through it what the reference binary printed -- on the seven
    hsp_softmask_* sets, and the codon restatement and the reference's recorded set on hsp_codon_softmask;
(c) equals what the reference binary printed under --seedrepeat 1, 2 and 3 (tests/golden/hsp_seedrepeat_*.jsonl,
    tools/make_seedrepeat_golden.py);
(d) and every generated case shows what its name claims, decided by replay_opt alone."""
import pytest

import exonerate_amd as ex
import hsp_codon_cases as hc
import seed_fused_cases as sf
import seed_fused_opt_cases as so
from golden_util import load_set
from test_hsp_softmask import SOFTMASK_SETS, Scorer, seed_set, word_hits
from test_oracle_seed import SEED_SETS, load_seed_set

RECORDS = [(name, k) for name in SEED_SETS for k in range(len(load_seed_set(name)))]
REPEAT_SETS = ["hsp_seedrepeat_dna2dna", "hsp_seedrepeat_protein2protein"]


@pytest.fixture(scope="module")
def params():
    return ex.default_params()


def test_the_engine_has_the_keywords():
    import inspect
    sig = inspect.signature(ex.Engine.seed_extend).parameters
    assert [sig[k].default for k in ("mask_query", "mask_target", "seed_repeat")] == [False, False, 1]


def test_all_records_are_here():
    assert len(RECORDS) == 25


@pytest.mark.parametrize("point", ["default", "low"])
@pytest.mark.parametrize("name,k", RECORDS)
def test_a_plain_replay_is_the_fused_yardstick(params, name, k, point):
    rec = load_seed_set(name)[k]
    dropoff, threshold = sf.points(rec["match"])[point]
    args = (params, rec["match"], rec["queries"], rec["target"], rec["expected"], rec["wordlen"], dropoff, threshold)
    assert so.replay_opt(*args) == sf.replay(*args)


@pytest.mark.parametrize("name", SOFTMASK_SETS)
def test_b_masked_replay_is_the_softmask_restatement(params, name):
    recs = load_set(name)
    par, recs = recs[0]["params"], recs[1:]
    n_dropped = 0
    for r in recs:
        for mq, mt, key in ((False, False, "plain"), (par["mask_query"], par["mask_target"], "masked")):
            seeds = word_hits(params, par, r["query"], r["target"], mq, mt)
            per_seed, exp = seed_set(Scorer(params, par["match"], r["query"], r["target"], mq, mt), par["seedlen"], par["dropoff"],
                                     par["threshold"], seeds)
            detail = {}
            kept, stats = so.replay_opt(params, par["match"], [r["query"]], r["target"], [[0, qs, ts] for qs, ts in seeds],
                                        par["seedlen"], par["dropoff"], par["threshold"], mq, mt, detail=detail)
            assert [h for _, _, h in kept] == exp, (r["id"], key)
            assert [v > 0 for v in detail["verdict"]] == [p is not None for p in per_seed], (r["id"], key)
            assert detail["dropped"] == [k for k, p in enumerate(per_seed) if p is not None and p[1]], (r["id"], key)
            assert stats["n_extended"] == sum(p is not None for p in per_seed) and stats["n_below"] == stats["n_extended"] - len(exp)
            mine = {tuple(h[:4]) for _, _, h in kept}                    # ... and through it the reference binary's own output
            assert all(tuple(h) in mine for h in r[key]) and (r[key] or not mine), (r["id"], key)
            n_dropped += len(detail["dropped"])
    assert n_dropped >= 6


def test_b_masked_codon_replay_is_the_codon_restatement(params):
    par, recs = hc.load_codon_set("hsp_codon_softmask")
    n_dropped = 0
    for r in recs:
        mq, mt = r["mask_query"], r["mask_target"]
        seeds = [tuple(s) for s in r["seeds"]]
        per_seed, exp = hc.seed_set(hc.CodonScorer(params, r["query"], r["target"], mq, mt), par["seedlen"], par["dropoff"],
                                    par["threshold"], seeds)
        detail = {}
        kept, stats = so.replay_opt(params, "codon2codon", [r["query"]], r["target"], [[0, qs, ts] for qs, ts in seeds], par["seedlen"],
                                    par["dropoff"], par["threshold"], mq, mt, detail=detail)
        assert [h for _, _, h in kept] == exp == r["set"], r["id"]
        assert [v > 0 for v in detail["verdict"]] == [p is not None for p in per_seed], r["id"]
        n_dropped += len(detail["dropped"])
    assert n_dropped >= 1


@pytest.mark.parametrize("name", REPEAT_SETS)
def test_c_replay_is_the_reference_binary_under_seedrepeat(params, name):
    """HSP for HSP what exonerate -m ungapped printed at --seedrepeat 1, 2 and 3 (forward strand), and the records decide:
    repeat 2 removes at least 6 HSPs, repeat 3 at least 3 more."""
    recs = load_set(name)
    par, recs = recs[0]["params"], recs[1:]
    count = {1: 0, 2: 0, 3: 0}
    for r in recs:
        for rep in (1, 2, 3):
            c = so.record_case(par, r, seed_repeat=rep)
            kept, _ = c.replay(params)
            assert sorted(h[:4] for _, _, h in kept) == r["repeat"][str(rep)], (r["id"], rep)
            count[rep] += len(kept)
    assert count[1] - count[2] >= 6 and count[2] - count[3] >= 3
    tag = [r for r in recs if r["id"] == "tag"][0]
    assert len(tag["repeat"]["1"]) == 2 and tag["repeat"]["2"] == []


def test_d_dropped_seed_lets_a_later_seed_of_its_entry_be_extended(params):
    c = so.case_dropped_then_extended()
    masked, plain = {}, {}
    kept, stats = c.replay(params, detail=masked)
    kept_plain, _ = c.replay(params, detail=plain, mask_target=False)
    later = [k for k, (_, qs, _) in enumerate(c.calls) if qs == 31]
    assert len(later) == 1 and c.calls[0][1:] == [0, 7]
    assert masked["dropped"] == [0] and masked["verdict"][later[0]] == 2 and plain["verdict"][later[0]] == 0
    assert [k for k, _, _ in kept] == later and [k for k, _, _ in kept_plain] == [0]
    assert kept[0][2][:3] == kept_plain[0][2][:3] == [0, 7, 60]                # the same HSP, from another seed
    assert stats["n_extended"] == 2 and stats["n_below"] == 1


def test_d_masked_run_keeps_fewer(params):
    c = so.case_masked_keeps_fewer()
    detail = {}
    kept, stats = c.replay(params, detail=detail)
    kept_plain, _ = c.replay(params, mask_target=False)
    assert [q for _, q, _ in kept] == [1] and sorted(q for _, q, _ in kept_plain) == [0, 1]
    assert len(detail["dropped"]) == 1


def test_d_tag_case(params):
    c = so.case_tag()
    assert len(c.calls) == 2 and c.calls[1][2] - c.calls[0][2] == len(c.queries[0]) and c.calls[0][1] == c.calls[1][1]
    assert so.entry_of("dna2dna", 100, *c.calls[0][1:]) == so.entry_of("dna2dna", 100, *c.calls[1][1:])
    assert c.replay(params)[1] == dict(n_hits=2, n_extended=0, n_below=0, n_kept=0)
    assert c.replay(params, tagless=True)[1]["n_kept"] == 1
    assert c.replay(params, seed_repeat=1)[1]["n_kept"] == 2


def test_d_codon_case_shares_an_entry_between_wrapped_diagonals(params):
    c = so.case_codon_wrapped_shared_entry()
    (_, qa, ta), (_, qb, tb) = c.calls
    assert hc.wrapped(90, qa, ta) and hc.wrapped(90, qb, tb) and ta - qa != tb - qb
    assert hc.entry(90, qa, ta) == hc.entry(90, qb, tb) == so.entry_of("codon2codon", 90, qb, tb)
    assert c.replay(params)[1]["n_extended"] == 0
    assert c.replay(params, tagless=True)[1]["n_kept"] == 1
    assert c.replay(params, seed_repeat=1)[1]["n_kept"] == 2


@pytest.mark.parametrize("match", ["dna2dna", "protein2protein"])
def test_d_counters(params, match):
    kept = {rep: [q for _, q, _ in so.case_counters(match, rep).replay(params)[0]] for rep in (1, 2, 3)}
    assert kept == {1: [0, 1, 2], 2: [1, 2], 3: [2]}
    assert [len([x for x in so.case_counters(match, 2).calls if x[0] == q]) for q in range(3)] == [1, 2, 3]


def test_d_masks_at_the_ends_and_single_lower_bases(params):
    c = so.case_mask_at_the_ends()
    kept, stats = c.replay(params)
    assert [h[:3] for _, _, h in kept] == [[0, 0, 61]] and c.target[0].islower() and c.target[-1].islower()
    assert stats["n_hits"] == 61 - 12 + 1 - 2                           # no word over the first or the last base
    for match in ("protein2dna", "codon2codon"):
        c = so.case_one_lower_base(match)
        assert sum(ch.islower() for ch in "".join(c.queries) + c.target) == 1
        kept, stats = c.replay(params)
        unflagged = so.Case(c.name, match, c.queries, c.target, c.wordlen, c.dropoff, c.threshold)
        assert stats["n_kept"] >= 1 and stats["n_hits"] < len(unflagged.calls)     # the words over the masked codon are gone


@pytest.mark.parametrize("name", [s[0] for s in sf.EDGE_SHAPES])
def test_d_edge_shapes(params, name):
    c = so.case_edge_opt(name)
    detail = {}
    kept, stats = c.replay(params, detail=detail)
    assert stats["n_kept"] >= 3 and stats["n_extended"] < stats["n_hits"] and detail["dropped"]
    assert (kept, stats) != c.replay(params, mask_target=False)
    c2 = so.case_edge_opt(name, seed_repeat=2)
    assert c2.replay(params) != c2.replay(params, seed_repeat=1) and c2.replay(params)[1]["n_kept"] >= 3
