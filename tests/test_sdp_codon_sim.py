"""The sparse SDP wavefront of coding2coding (exonerate_amd/csrc/c4_sdp_wave.h with a query advance of up to 3: per-lane cell
function, one ring per hop, three carried rows per strip, the dead-run rule, streams, the walk; c4_sdp_host.h) driven by CPU
loops (tests/sdp_codon_sim.hip) against the reference's own SDP alignments (tests/golden/sdp_coding2coding*.jsonl), against
the oracle on the strip-edge bands (tests/sdp_codon_cases.py) and on a seeded fuzz.  No GPU involved: this checks the
algorithm the kernels implement; tests/test_gpu_sdp_codon.py checks the kernels themselves."""
import pytest

import sdp_codon_cases as sc
import sdp_codon_sim_lib
from test_oracle_sdp_codon import ADV, CODON_SDP_SETS, codon_sdp_case, expected

KEYS = ("score", "region", "ops", "vulgar")


@pytest.mark.parametrize("name", sorted(CODON_SDP_SETS))
def test_simulated_wavefront_matches_reference_vectors(name):
    model, par, recs = codon_sdp_case(name)
    total = 0
    for r in recs:
        got, steps = sdp_codon_sim_lib.sdp(model.c, model.params, r["query"].encode(), r["target"].encode(), r["hsps"], ADV[0], ADV[1],
                                           par["dropoff"], par["threshold"], 4, qid=r["id"])
        assert [{k: a[k] for k in KEYS} for a in got] == expected(r), r["id"]
        total += len(got)
    assert total >= 10


@pytest.mark.parametrize("k", sc.BANDS + ("small",))
def test_simulated_wavefront_on_the_strip_edge_bands(k):
    threshold = 10 if k == "small" else sc.THRESHOLD
    for point, dropoff, pair in sc.band_runs(k):
        model = sc.model_at(point)
        hsps = sc.hsps_of(model.params, pair)
        exp = sc.oracle_sdp(model, pair["q"], pair["t"], hsps, (3, 3), dropoff, threshold)
        got, steps = sdp_codon_sim_lib.sdp(model.c, model.params, pair["q"].encode(), pair["t"].encode(), hsps, 3, 3, dropoff, threshold, 4)
        assert got == exp, (k, point, dropoff, pair["kind"], pair["row"], pair["mirrored"])
        assert exp


@pytest.mark.parametrize("seed", range(4))
def test_simulated_wavefront_seeded_fuzz(seed):
    n = 0
    seen = set()
    for cs in sc.fuzz_cases(seed):
        model, adv = cs["model"], cs["adv"]
        for (q, t), h in zip(cs["pairs"], cs["hsps"]):
            exp = sc.oracle_sdp(model, q, t, h, adv, cs["dropoff"], cs["threshold"])
            got, steps = sdp_codon_sim_lib.sdp(model.c, model.params, q.encode(), t.encode(), h, adv[0], adv[1], cs["dropoff"], cs["threshold"], 4)
            assert got == exp, (seed, cs["point"], adv, cs["dropoff"], cs["threshold"], len(q), len(t), len(h))
            n += len(exp)
        seen.add((adv, cs["dropoff"]))
    assert n >= 2 and len(seen) >= 2
