"""The extension of one HSP seed and the horizon step the device kernels loop around (exonerate_amd/csrc/c4_hsp_extend.h),
compiled for the host (tests/hsp_sim.hip) and held, without a GPU, to what the device tests hold the kernels to: the
reference's recorded per-seed and whole-set HSPs with masks off (tests/golden/hsp_*.jsonl), and the Python restatement of
test_hsp_softmask.py on the recorded soft-masked pairs and on the seeded random families of test_gpu_hsp_softmask.py (same
generator seeds: the host test and the GPU test see the same cases)."""
import random
import pytest

import hsp_sim_lib
from golden_util import load_set
from test_oracle_hsp import HSP_SETS
from test_hsp_softmask import SOFTMASK_SETS, Scorer, seed_hsp, seed_set, word_hits
from test_gpu_hsp_softmask import random_pairs


@pytest.mark.parametrize("name", HSP_SETS)
def test_recorded_hsps_with_masks_off(params, name):
    recs = load_set(name)
    par, recs = recs[0]["params"], recs[1:]
    assert par["seed_repeat"] == 1
    ext = par["seedlen"], par["dropoff"], par["threshold"]
    for r in recs:
        pair = hsp_sim_lib.Pair(params, par["match"], r["query"], r["target"])
        for (qs, ts), exp in zip(r["seeds"], r["single"]):
            got, dropped = pair.seed(*ext, qs, ts)
            assert not dropped
            if exp is None:
                assert got[3] < par["threshold"], (r["id"], qs, ts)
            else:
                assert got == exp, (r["id"], qs, ts)
        walked = pair.walk(*ext, [tuple(s) for s in r["seeds"]])
        assert [w[0] for w in walked if w is not None and w[0][3] >= par["threshold"]] == r["set"], r["id"]


def check_against_restatement(params, match, pairs, seeds, seedlen, dropoff, threshold, mq, mt):
    """As check_against_restatement of test_gpu_hsp_softmask.py holds the device: every seed on its own against seed_hsp, the
    walk of each pair's seeds against seed_set (skips, HSPs, dropped flags, the kept list).  seeds: per pair its (qs, ts).
    Returns the numbers of dropped and of skipped seeds of the walks."""
    n_dropped = n_skipped = 0
    for (q, t), mine in zip(pairs, seeds):
        sc = Scorer(params, match, q, t, mq, mt)
        pair = hsp_sim_lib.Pair(params, match, q, t, mq, mt)
        for qs, ts in mine:
            assert pair.seed(seedlen, dropoff, threshold, qs, ts) == seed_hsp(sc, seedlen, dropoff, threshold, qs, ts), (q, t, qs, ts)
        per_seed, exp_kept = seed_set(sc, seedlen, dropoff, threshold, mine)
        walked = pair.walk(seedlen, dropoff, threshold, mine)
        assert walked == per_seed, (q, t)
        assert [h for h, dropped in filter(None, walked) if not dropped and h[3] >= threshold] == exp_kept
        n_dropped += sum(1 for w in walked if w is not None and w[1])
        n_skipped += sum(1 for w in walked if w is None)
    return n_dropped, n_skipped


@pytest.mark.parametrize("name", SOFTMASK_SETS)
def test_recorded_softmasked_pairs(params, name):
    recs = load_set(name)
    par, recs = recs[0]["params"], recs[1:]
    mq, mt = par["mask_query"], par["mask_target"]
    pairs = [(r["query"], r["target"]) for r in recs]
    seeds = [word_hits(params, par, q, t, mq, mt) for q, t in pairs]
    n_dropped, n_skipped = check_against_restatement(params, par["match"], pairs, seeds, par["seedlen"], par["dropoff"],
                                                     par["threshold"], mq, mt)
    assert n_dropped >= 6 and n_skipped >= 1


@pytest.mark.parametrize("match,seedlen,dropoff,threshold", [("dna2dna", 8, 12, 50), ("protein2protein", 3, 9, 22),
                                                             ("protein2dna", 3, 9, 22)])
@pytest.mark.parametrize("mq,mt", [(False, True), (True, False), (True, True)])
def test_random_small_pairs(params, match, seedlen, dropoff, threshold, mq, mt):
    rng = random.Random(1000 * mq + 100 * mt + len(match))
    pairs = random_pairs(rng, match, 300)
    par = {"match": match, "seedlen": seedlen}
    seeds = [word_hits(params, par, q, t, False, False) for q, t in pairs]
    n_dropped, n_skipped = check_against_restatement(params, match, pairs, seeds, seedlen, dropoff, threshold, mq, mt)
    assert n_dropped > 100 and n_skipped > 100
