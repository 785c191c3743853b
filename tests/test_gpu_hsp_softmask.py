"""The two-stage HSP extension of soft-masked sets on the device (c4gpu_hsp_extend_batch_masked / _chains_masked,
hspset.c:981-995) against the Python restatement of test_hsp_softmask.py, seed for seed: on the pairs recorded from the
reference binary (tests/golden/hsp_softmask_*.jsonl) and on seeded random small pairs of every match kind; kept ends, score
and cobs, the dropped flag and the masked end; the chain form against the batch form plus a host replay of the horizon; with
both flags 0 against the old entry points; and, one-directionally, against the reference's recorded HSP lines."""
import random
import pytest

import exonerate_amd as ex
from golden_util import load_set
from test_hsp_softmask import SOFTMASK_SETS, ADVANCE, Scorer, seed_hsp, seed_set, word_hits

pytestmark = pytest.mark.gpu

AA = "ARNDCQEGHILKMFPSTWYV"
TABLE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODON = {}
for _i, _a in enumerate("TCAG"):
    for _j, _b in enumerate("TCAG"):
        for _k, _c in enumerate("TCAG"):
            CODON.setdefault(TABLE[_i * 16 + _j * 4 + _k], []).append(_a + _b + _c)


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


def chains_of(pairs, seeds, at):
    keys, chain = {}, []
    for k, qs, ts in seeds:
        n = len(pairs[k][0])
        chain.append(keys.setdefault((k, (ts - qs * at + n) % n, ts % at), len(keys)))
    return chain, len(keys)


def check_against_restatement(eng, params, match, pairs, seeds, seedlen, dropoff, threshold, mq, mt):
    """Batch form seed for seed; chain form = batch form + a host replay of the horizon = the restatement's whole-set walk.
    Returns the kept HSPs per pair (chain form) and the number of dropped seeds."""
    at = ADVANCE[match][1]
    scorers = [Scorer(params, match, q, t, mq, mt) for q, t in pairs]
    got = eng.hsp_extend_masked(params, match, pairs, seedlen, dropoff, seeds, mq, mt, threshold)
    assert len(got) == len(seeds)
    for (k, qs, ts), (h, dropped) in zip(seeds, got):
        exp, exp_dropped = seed_hsp(scorers[k], seedlen, dropoff, threshold, qs, ts)
        assert (h, dropped) == (exp, exp_dropped), (pairs[k], qs, ts)
    chain, n_chains = chains_of(pairs, seeds, at)
    cgot = eng.hsp_extend_chains_masked(params, match, pairs, seedlen, dropoff, seeds, chain, [0] * n_chains, mq, mt, threshold)
    horizon = [0] * n_chains
    kept = [[] for _ in pairs]
    n_dropped = n_skipped = 0
    for (k, qs, ts), c, (h, dropped), (b, b_dropped) in zip(seeds, chain, cgot, got):
        if ts < horizon[c]:                                  # the replay's decision from the batch form's numbers
            assert h[2] == -1 and dropped == 0, (pairs[k], qs, ts)
            n_skipped += 1
            continue
        assert (h, dropped) == (b, b_dropped), (pairs[k], qs, ts)
        horizon[c] = h[1] + h[2] * at
        if dropped:
            n_dropped += 1
        elif h[3] >= threshold:
            kept[k].append(h)
    # ... and the restatement's own walk, pair by pair
    pos = 0
    for k, sc in enumerate(scorers):
        mine = [(qs, ts) for kk, qs, ts in seeds if kk == k]
        per_seed, exp_kept = seed_set(sc, seedlen, dropoff, threshold, mine)
        for e, (h, dropped) in zip(per_seed, cgot[pos:pos + len(mine)]):
            assert (e is None and h[2] == -1 and not dropped) or e == (h, dropped)
        assert kept[k] == exp_kept
        pos += len(mine)
    return kept, n_dropped, n_skipped


@pytest.mark.parametrize("name", SOFTMASK_SETS)
def test_recorded_pairs(eng, name):
    recs = load_set(name)
    par, recs = recs[0]["params"], recs[1:]
    params = ex.default_params()
    pairs = [(r["query"], r["target"]) for r in recs]
    mq, mt = par["mask_query"], par["mask_target"]
    seeds = [(k, qs, ts) for k, r in enumerate(recs) for qs, ts in word_hits(params, par, r["query"], r["target"], mq, mt)]
    assert len(seeds) > 50
    kept, n_dropped, n_skipped = check_against_restatement(eng, params, par["match"], pairs, seeds, par["seedlen"], par["dropoff"],
                                                           par["threshold"], mq, mt)
    assert n_dropped >= 6 and n_skipped > 0
    # one-directional: every HSP the reference binary printed with the option(s) is there; nothing for a pair it dropped
    for r, ks in zip(recs, kept):
        mine = [h[:4] for h in ks]
        for h in r["masked"]:
            assert h in mine, (r["id"], h, mine)
        if not r["masked"]:
            assert not mine, (r["id"], mine)
    # both flags 0: the old entry points, lower case or not (a soft-masked run without the option is a plain run)
    old = eng.hsp_extend(params, par["match"], pairs, par["seedlen"], par["dropoff"], seeds)
    new = eng.hsp_extend_masked(params, par["match"], pairs, par["seedlen"], par["dropoff"], seeds, False, False, par["threshold"])
    assert [h for h, d in new] == old and not any(d for h, d in new)
    chain, n_chains = chains_of(pairs, seeds, par["target_advance"])
    old = eng.hsp_extend_chains(params, par["match"], pairs, par["seedlen"], par["dropoff"], seeds, chain, [0] * n_chains)
    new = eng.hsp_extend_chains_masked(params, par["match"], pairs, par["seedlen"], par["dropoff"], seeds, chain, [0] * n_chains,
                                       False, False, par["threshold"])
    assert [h for h, d in new] == old and not any(d for h, d in new)


def random_case(rng, s, p_run):
    """Runs of lower case over s; now and then the wildcard in lower case, which is NOT masked (alphabet.c:124-129)."""
    out, low = [], False
    for c in s:
        if rng.random() < p_run:
            low = not low
        out.append(c.lower() if low else c)
    return "".join(out)


def random_pairs(rng, match, n):
    pairs = []
    for _ in range(n):
        if match == "dna2dna":
            q = "".join(rng.choice("ACGT") for _ in range(rng.randint(20, 70)))
            body = "".join(rng.choice("ACGTN") if rng.random() < 0.06 else c for c in q)
            pad = lambda: "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 12)))
        else:
            q = "".join(rng.choice(AA) for _ in range(rng.randint(10, 30)))
            body = "".join(rng.choice(AA + "X") if rng.random() < 0.08 else c for c in q)
            if match == "protein2dna":
                body = "".join(rng.choice(CODON[a]) if a != "X" else "NNN" for a in body)
                pad = lambda: "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 7)))
            else:
                pad = lambda: "".join(rng.choice(AA) for _ in range(rng.randint(0, 6)))
        t = pad() + body[rng.randint(0, 4) * (3 if match == "protein2dna" else 1):] + pad()
        pairs.append((random_case(rng, q, 0.12), random_case(rng, t, 0.1)))
    return pairs


@pytest.mark.parametrize("match,seedlen,dropoff,threshold", [("dna2dna", 8, 12, 50), ("protein2protein", 3, 9, 22),
                                                             ("protein2dna", 3, 9, 22)])
@pytest.mark.parametrize("mq,mt", [(False, True), (True, False), (True, True)])
def test_random_small_pairs(eng, match, seedlen, dropoff, threshold, mq, mt):
    """300 pairs per match kind and flag combination, every shared word (masked or not: a seed is a pair of positions) as a
    seed, in one launch: masks against the seed, at either end of a sequence, in every codon position, on either side."""
    rng = random.Random(1000 * mq + 100 * mt + len(match))
    params = ex.default_params()
    pairs = random_pairs(rng, match, 300)
    par = {"match": match, "seedlen": seedlen}
    seeds = [(k, qs, ts) for k, (q, t) in enumerate(pairs) for qs, ts in word_hits(params, par, q, t, False, False)]
    assert len(seeds) > 1500
    kept, n_dropped, n_skipped = check_against_restatement(eng, params, match, pairs, seeds, seedlen, dropoff, threshold, mq, mt)
    assert n_dropped > 100 and n_skipped > 100 and sum(len(k) for k in kept) > 50


def test_seed_outside_its_pair_is_rejected(eng):
    with pytest.raises(ex.C4GpuError):
        eng.hsp_extend_masked(ex.default_params(), "dna2dna", [("ACGTACGTACGTACGT", "acgtACGTACGTACGT")], 12, 30, [(0, 8, 0)],
                              False, True, 75)
