"""HSP seeding of the translated models (C4GPU_MATCH_CODON2CODON) without a GPU: the Python restatement for the codon match
(hsp_codon_cases.py: codon rows on both sides, advances 3/3, the horizon entry in the reference's unsigned arithmetic) and the
product's own extension routine compiled for the host (c4_hsp_extend.h through hsp_codon_sim_lib.py) are each held to every
per-seed record and every whole set the reference's own functions produced for codon sets (tests/golden/hsp_codon.jsonl,
hsp_codon_softmask.jsonl: tools/make_codon_hsp_golden.py); and the fixtures are held to what they must cover.  The device entry
points are held to the same records in test_gpu_hsp_codon.py."""
import json
import os

import pytest

import hsp_codon_cases as hc
from golden_util import GOLDEN_DIR
from test_hsp_softmask import seed_hsp


def _restatement(params, rec):
    sc = hc.CodonScorer(params, rec["query"], rec["target"], rec["mask_query"], rec["mask_target"])
    return (lambda par, qs, ts: seed_hsp(sc, par["seedlen"], par["dropoff"], par["threshold"], qs, ts),
            lambda par, seeds: hc.seed_set(sc, par["seedlen"], par["dropoff"], par["threshold"], seeds)[0])


def _product(params, rec):
    import hsp_codon_sim_lib
    p = hsp_codon_sim_lib.CodonPair(params, rec["query"], rec["target"], rec["mask_query"], rec["mask_target"])
    return (lambda par, qs, ts: p.seed(par["seedlen"], par["dropoff"], par["threshold"], qs, ts),
            lambda par, seeds: p.walk(par["seedlen"], par["dropoff"], par["threshold"], [tuple(s) for s in seeds]))


ROUTES = {"restatement": _restatement, "product": _product}


def check_single(par, rec, k, got, dropped):
    """One seed's answer against the record (also used by the GPU tests)."""
    exp, end = rec["single"][k], rec["dropped_end"][k]
    where = (rec["id"], rec["seeds"][k])
    if end is not None:                                    # dropped: the masked end is what the horizon entry receives
        assert dropped and got[1] + got[2] * 3 == end and got[4] == 0, where
    elif exp is None:                                      # a plain set: grown, and below the threshold (HSP_store)
        assert not dropped and got[3] < par["threshold"] and not (rec["mask_query"] or rec["mask_target"]), where
    else:
        assert not dropped and got == exp, where


def kept_of(par, per_seed):
    return [h for x in per_seed if x is not None for h, d in [x] if not d and h[3] >= par["threshold"]]


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("name", hc.CODON_SETS)
def test_every_record_and_every_set(params, name, route):
    par, recs = hc.load_codon_set(name)
    assert (par["match"], par["query_advance"], par["target_advance"], par["seed_repeat"]) == ("codon2codon", 3, 3, 1)
    assert len(recs) >= 2
    for rec in recs:
        single, walk = ROUTES[route](params, rec)
        for k, (qs, ts) in enumerate(rec["seeds"]):
            got, dropped = single(par, qs, ts)
            check_single(par, rec, k, got, dropped)
        per_seed = walk(par, rec["seeds"])
        assert kept_of(par, per_seed) == rec["set"], rec["id"]
        if route == "product":                             # ... and seed for seed what the restatement's walk does
            assert per_seed == _restatement(params, rec)[1](par, rec["seeds"]), rec["id"]


def test_the_seed_extend_yardstick_gives_the_recorded_sets(params):
    """codon_seed_cases.replay (what test_gpu_seed_extend_codon.py holds c4gpu_seed_extend to) over the recorded scans."""
    import codon_seed_cases
    par, recs = hc.load_codon_set("hsp_codon")
    for rec in recs:
        kept, stats = codon_seed_cases.replay(params, [rec["query"]], rec["target"], [[0, qs, ts] for qs, ts in rec["seeds"]],
                                              par["seedlen"], par["dropoff"], par["threshold"])
        assert [h for _, _, h in kept] == rec["set"], rec["id"]
        assert stats["n_hits"] == len(rec["seeds"]) and stats["n_extended"] == stats["n_below"] + stats["n_kept"]


def test_the_signed_key_would_not_do(params):
    """Keyed with C's signed remainder (no entry for a negative sum, as the 1/1 and 1/3 forms have it) some recorded set comes
    out different: the wrapped seeds are tested against, and move, an entry another diagonal owns."""
    differ = 0
    for name in hc.CODON_SETS:
        par, recs = hc.load_codon_set(name)
        for rec in recs:
            sc = hc.CodonScorer(params, rec["query"], rec["target"], rec["mask_query"], rec["mask_target"])
            horizon, kept = {}, []
            for qs, ts in rec["seeds"]:
                key = None if hc.wrapped(sc.qlen, qs, ts) else hc.entry(sc.qlen, qs, ts)
                if key is not None and ts < horizon.get(key, 0):
                    continue
                h, dropped = seed_hsp(sc, par["seedlen"], par["dropoff"], par["threshold"], qs, ts)
                if key is not None:
                    horizon[key] = h[1] + h[2] * 3
                if not dropped and h[3] >= par["threshold"]:
                    kept.append(h)
            differ += kept != rec["set"]
    assert differ > 0


def coverage(params):
    """What the two files hold, as numbers (tools/make_codon_hsp_golden.py prints the same)."""
    cov = dict(frames=set(), wrapped_shared=0, skipped=0, dropped=0, trim_start=0, trim_end=0, q_ends=set(), t_ends=set(),
               q_start0=0, t_start0=0)
    for name in hc.CODON_SETS:
        par, recs = hc.load_codon_set(name)
        for rec in recs:
            sc = hc.CodonScorer(params, rec["query"], rec["target"], rec["mask_query"], rec["mask_target"])
            owners = {}
            for qs, ts in rec["seeds"]:
                cov["frames"].add((qs % 3, ts % 3))
                owners.setdefault(hc.entry(sc.qlen, qs, ts), set()).add(ts - qs)
                cov["trim_start"] += sc.score(qs, ts) <= 0
                cov["trim_end"] += sc.score(qs + 3 * (par["seedlen"] - 1), ts + 3 * (par["seedlen"] - 1)) <= 0
            cov["wrapped_shared"] += sum(1 for qs, ts in rec["seeds"]
                                         if hc.wrapped(sc.qlen, qs, ts) and len(owners[hc.entry(sc.qlen, qs, ts)]) > 1)
            cov["skipped"] += sum(x is None for x in hc.seed_set(sc, par["seedlen"], par["dropoff"], par["threshold"], rec["seeds"])[0])
            if name == "hsp_codon_softmask":
                cov["dropped"] += sum(e is not None for e in rec["dropped_end"])
            for h in [h for h in rec["single"] if h] + rec["set"]:
                cov["q_start0"] += h[0] == 0
                cov["t_start0"] += h[1] == 0
                cov["q_ends"].add(sc.qlen - (h[0] + 3 * h[2]))
                cov["t_ends"].add(sc.tlen - (h[1] + 3 * h[2]))
    return cov


def test_the_fixtures_cover_what_they_must(params):
    cov = coverage(params)
    assert cov["frames"] == {(a, b) for a in range(3) for b in range(3)}          # all nine (query frame, target frame) pairs
    assert cov["wrapped_shared"] >= 1                  # a wrapped seed whose entry another diagonal uses too
    assert cov["skipped"] >= 1                         # a seed under its horizon
    assert cov["dropped"] >= 6                         # seeds dropped at masked ends, in the masked file
    assert cov["trim_start"] >= 1 and cov["trim_end"] >= 1
    assert cov["q_start0"] and cov["t_start0"]         # HSPs that reach position 0 ...
    assert {0, 1, 2} <= cov["q_ends"] and {0, 1, 2} <= cov["t_ends"]              # ... and len, len - 1, len - 2 of each sequence


def test_the_cli_fixture_names_the_same_inputs():
    """codon_hsp_cli.json: the inputs and the reference binary's sugar lines of the runs the sets were recorded from."""
    with open(os.path.join(GOLDEN_DIR, "codon_hsp_cli.json")) as f:
        cli = json.load(f)["runs"]
    seqs = {(r["query"], r["target"]) for n in hc.CODON_SETS for r in hc.load_codon_set(n)[1]}
    comp = str.maketrans("ACGTacgt", "TGCAtgca")
    for name, run in cli.items():
        assert len(run["query"]) <= 300 and run["sugar"], name
        strands = lambda s: {s, s.translate(comp)[::-1]}
        assert any(q in strands(run["query"]) and t in strands(run["target"]) for q, t in seqs), name
        for line in run["sugar"]:
            f = line.split()
            assert f[0] == "sugar:" and f[1] == "qy" and f[5] == "tg" and int(f[9]) > 0
