"""The sparse SDP wavefront of coding2genome (exonerate_amd/csrc/c4_sdp_wave.h: the boundary flavour at a query advance of up to
3 -- one ring per hop with its shadow word, three carried rows per strip, forward strips anchored at the query's end, mirrored
boundary records, span stores, the split-codon calc of a DNA query, the walk; c4_sdp_host.h) driven by CPU loops
(tests/sdp_c2g_sim.hip) against the reference's own SDP alignments (all four sets of tests/golden/sdp_coding2genome*.jsonl,
split codons included) and, on a seeded fuzz without introns of phase 1 or 2, against the oracle.  No GPU involved: this checks
the algorithm the kernels implement; tests/test_gpu_sdp_coding2genome.py checks the kernels themselves."""
import pytest

import oracle_lib
import sdp_c2g_cases as sc
import sdp_c2g_sim_lib
import sdp_codon_cases


@pytest.mark.parametrize("name", sorted(sc.SDP_SETS))
def test_simulated_wavefront_matches_reference_vectors(name):
    model, par, recs = sc.sdp_case(name)
    total = 0
    for r in recs:
        got, steps = sdp_c2g_sim_lib.sdp(model.c, model.params, r["query"].encode(), r["target"].encode(), r["hsps"], sc.ADV[0], sc.ADV[1],
                                         par["dropoff"], par["threshold"], 4, qid=r["id"])
        assert [{k: a[k] for k in sc.KEYS} for a in got] == sc.expected(r), r["id"]
        total += len(got)
    assert total >= 10


@pytest.mark.parametrize("seed", range(4))
def test_simulated_wavefront_seeded_fuzz(seed):
    model, _, _ = sc.sdp_case(("sdp_coding2genome", "sdp_coding2genome_altparams")[seed % 2])
    dropoff, threshold = (50, 5)[seed // 2], (40, 30)[seed // 2]
    n = introns = 0
    for q, t in sc.fuzz_pairs(seed, 8):
        hsps = sdp_codon_cases._dna_hsps(model.params, q, t)
        if not hsps:
            continue
        ub, exp = oracle_lib.sdp(model.c, model.params, q.encode(), t.encode(), hsps, 1, 1, dropoff, True, threshold, 4)
        assert ub == 1
        if any(tr in sc.SPLIT_POST for a in exp for tr, _ in a["ops"]):
            continue                                              # a split codon after all: not the oracle's to judge
        got, steps = sdp_c2g_sim_lib.sdp(model.c, model.params, q.encode(), t.encode(), hsps, 1, 1, dropoff, threshold, 4)
        assert got == exp, (seed, len(q), len(t), len(hsps))
        n += len(exp)
        introns += sum(len(sc.intron_phases(model, a)) for a in exp)
    # at a dropoff of 5 no path crosses an intron (its 5' transition alone costs more): the seeds at 50 must show one
    assert n >= 4 and (introns >= 1 or dropoff == 5)
