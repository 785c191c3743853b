"""The four c4gpu_hsp_extend_* entry points with C4GPU_MATCH_CODON2CODON (both advances 3, codon rows on both sides, either
side's soft mask over the three bases of a codon) against the reference's recorded codon sets (tests/golden/hsp_codon*.jsonl) and
the Python restatement of hsp_codon_cases.py, seed for seed: one pair, three pairs that share one query buffer, three pairs with
distinct queries, 1 / 63 / 64 / 65 horizon chains (one lane per chain, 64 lanes per block), each mask flag alone and both."""
import pytest

import exonerate_amd as ex
import hsp_codon_cases as hc
from test_hsp_codon import check_single
from test_hsp_softmask import seed_hsp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def params():
    return ex.default_params()


@pytest.fixture(scope="module")
def golden():
    """(params, {record id: record}) of both files."""
    par, plain = hc.load_codon_set("hsp_codon")
    par2, soft = hc.load_codon_set("hsp_codon_softmask")
    assert par == par2
    return par, {r["id"]: r for r in plain + soft}


def chains_of(pairs, seeds):
    keys, chain = {}, []
    for k, qs, ts in seeds:
        chain.append(keys.setdefault((k,) + hc.entry(len(pairs[k][0]), qs, ts), len(keys)))
    return chain, len(keys)


def run_both_forms(eng, params, par, pairs, seeds, mq, mt):
    """(batch form, chain form), each [(hsp, dropped)] per seed: the plain entry points without a flag, the masked ones with."""
    chain, n_chains = chains_of(pairs, seeds)
    a = (params, "codon2codon", pairs, par["seedlen"], par["dropoff"], seeds)
    if mq or mt:
        return (eng.hsp_extend_masked(*a, mq, mt, par["threshold"]),
                eng.hsp_extend_chains_masked(*a, chain, [0] * n_chains, mq, mt, par["threshold"])), chain, n_chains
    return ([(h, 0) for h in eng.hsp_extend(*a)], [(h, 0) for h in eng.hsp_extend_chains(*a, chain, [0] * n_chains)]), chain, n_chains


def check_against_restatement(eng, params, par, pairs, seeds, mq=False, mt=False):
    """Batch form seed for seed against the restatement's single seed; chain form seed for seed against the restatement's
    whole-set walk, pair by pair.  Returns the kept HSPs per pair and the numbers of dropped and skipped seeds."""
    scorers = [hc.CodonScorer(params, q, t, mq, mt) for q, t in pairs]
    (got, cgot), chain, n_chains = run_both_forms(eng, params, par, pairs, seeds, mq, mt)
    assert len(got) == len(cgot) == len(seeds)
    for (k, qs, ts), (h, dropped) in zip(seeds, got):
        assert (h, dropped) == seed_hsp(scorers[k], par["seedlen"], par["dropoff"], par["threshold"], qs, ts), (k, qs, ts)
    kept, n_dropped, n_skipped = [[] for _ in pairs], 0, 0
    for k, sc in enumerate(scorers):
        at = [x for x, s in enumerate(seeds) if s[0] == k]
        per_seed, exp_kept = hc.seed_set(sc, par["seedlen"], par["dropoff"], par["threshold"], [seeds[x][1:] for x in at])
        for x, e in zip(at, per_seed):
            h, dropped = cgot[x]
            if e is None:
                assert h[2] == -1 and dropped == 0, seeds[x]
                n_skipped += 1
            else:
                assert e == (h, dropped), seeds[x]
                n_dropped += dropped
                if not dropped and h[3] >= par["threshold"]:
                    kept[k].append(h)
        assert kept[k] == exp_kept
    return kept, n_dropped, n_skipped, n_chains


def seeds_of(recs):
    return [(k, qs, ts) for k, r in enumerate(recs) for qs, ts in r["seeds"]]


def test_one_pair_every_record(eng, params, golden):
    """Each recorded set as a launch of its own, with the flags it was recorded under: per seed the reference's own answer,
    and the chain form's kept list is the set the reference held."""
    par, recs = golden
    n_dropped = 0
    for rec in recs.values():
        pairs, seeds = [(rec["query"], rec["target"])], seeds_of([rec])
        mq, mt = rec["mask_query"], rec["mask_target"]
        (got, _), _, _ = run_both_forms(eng, params, par, pairs, seeds, mq, mt)
        for k, (h, dropped) in enumerate(got):
            check_single(par, rec, k, h, dropped)
        kept, d, n_skipped, _ = check_against_restatement(eng, params, par, pairs, seeds, mq, mt)
        assert kept[0] == rec["set"], rec["id"]
        n_dropped += d
    assert n_dropped >= 6


def test_three_pairs_sharing_one_query_buffer(eng, params, golden):
    par, recs = golden
    mine = [recs["A_0"], recs["C_0"], recs["B_t_0"]]
    q = mine[0]["query"]
    assert all(r["query"] == q for r in mine)
    pairs = [(q, r["target"]) for r in mine]                 # one object: one device copy, translated once
    kept, _, n_skipped, _ = check_against_restatement(eng, params, par, pairs, seeds_of(mine))
    assert kept[0] == mine[0]["set"] and kept[1] == mine[1]["set"] and kept[2] and n_skipped > 0


def test_three_pairs_with_distinct_queries(eng, params, golden):
    par, recs = golden
    mine = [recs["A_0"], recs["D_0"], recs["E_0"]]
    assert len({r["query"] for r in mine}) == 3 and len({len(r["query"]) % 4 for r in mine}) > 1
    pairs = [(r["query"], r["target"]) for r in mine]
    kept, _, n_skipped, _ = check_against_restatement(eng, params, par, pairs, seeds_of(mine))
    assert [kept[k] for k in range(3)] == [r["set"] for r in mine] and n_skipped > 0


@pytest.mark.parametrize("n_chains", [1, 63, 64, 65])
def test_chain_counts(eng, params, golden, n_chains):
    """The word hits of a generated scan (four queries against one target, codon_seed_cases.case_hits) in walk order, those of
    a new chain left out once `n_chains` are open; the first eight of every chain."""
    import codon_seed_cases
    par, _ = golden
    c = codon_seed_cases.case_hits(2047, par["seedlen"], par["dropoff"], par["threshold"])
    open_, seeds = {}, []
    for s in c.calls:
        key = (s[0],) + hc.entry(len(c.queries[s[0]]), s[1], s[2])
        if (key in open_ or len(open_) < n_chains) and open_.get(key, 0) < 8:
            open_[key] = open_.get(key, 0) + 1
            seeds.append(tuple(s))
    kept, _, n_skipped, got_chains = check_against_restatement(eng, params, par, c.pairs, seeds)
    assert got_chains == n_chains and len(seeds) > n_chains and sum(len(k) for k in kept) > 0
    assert n_chains == 1 or n_skipped > 0


def lower_islands(seq, spans):
    return "".join(c.lower() if any(a <= i < b for a, b in spans) else c for i, c in enumerate(seq))


@pytest.mark.parametrize("mq,mt", [(True, False), (False, True), (True, True)])
def test_mask_flags(eng, params, golden, mq, mt):
    """The soft-masked pair of the fixtures (lower-case target) with lower-case runs in the query as well -- across codon
    boundaries, so that a codon is masked by its first, second or third base alone: each flag alone masks its own side only."""
    par, recs = golden
    rec = recs["B_t_0"]
    q = lower_islands(rec["query"], [(0, 27), (45, 90), (103, 131), (200, 203), (250, 266)])      # [27, 45), [90, 103): short islands
    pairs, seeds = [(q, rec["target"])], seeds_of([rec])
    kept, n_dropped, n_skipped, _ = check_against_restatement(eng, params, par, pairs, seeds, mq, mt)
    assert n_dropped > 0 and n_skipped > 0 and kept[0]
    if not mq:                                             # the query's case is then not read: the recorded run itself
        assert kept[0] == rec["set"]
    # with both flags off the masked entry points are the plain ones: lower case or not, nothing dropped
    a = (params, "codon2codon", pairs, par["seedlen"], par["dropoff"], seeds)
    off = eng.hsp_extend_masked(*a, False, False, par["threshold"])
    assert [h for h, d in off] == eng.hsp_extend(*a) and not any(d for h, d in off)


def test_refusals(eng, params, golden):
    par, recs = golden
    rec = recs["A_0"]
    pairs = [(rec["query"], rec["target"])]
    qlen, tlen, n = len(rec["query"]), len(rec["target"]), par["seedlen"]
    ok = [(0, qlen - 3 * n, 0), (0, 0, tlen - 3 * n)]      # the last seed that fits on either side: seedlen * 3 bases
    assert len(eng.hsp_extend(params, "codon2codon", pairs, n, par["dropoff"], ok)) == 2
    for bad in [(0, qlen - 3 * n + 1, 0), (0, 0, tlen - 3 * n + 1)]:
        with pytest.raises(ex.C4GpuError, match="outside its pair"):
            eng.hsp_extend(params, "codon2codon", pairs, n, par["dropoff"], [bad])
    # match type 7 (and 4, the first number past the enum) is still none: refused before anything is read
    for kind in (7, 4):
        assert ex._lib().c4gpu_hsp_extend_batch(eng.ctx, params, kind, None, 0, n, par["dropoff"], None, 0, None) == -1
        assert "unknown match type" in str(ex._err("c4gpu_hsp_extend_batch"))
