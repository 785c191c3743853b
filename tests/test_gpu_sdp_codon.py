"""coding2coding's SDP on the device (c4gpu_sdp_batch: both Scheduler passes of the seeded flavour as sparse wavefronts whose
lanes exchange up to three query rows per step, c4_sdp_wave.h) through Engine.sdp: against the reference's own SDP alignments
(tests/golden/sdp_coding2coding*.jsonl), against the oracle on the strip-edge bands and a seeded fuzz (tests/sdp_codon_cases.py),
on a batch that mixes one to five strips with a pair without HSPs, and with an arena too small for some pairs.  A pair that
comes back unserved (None) is a failure here."""
import random

import pytest

import exonerate_amd as ex
import sdp_codon_cases as sc
from test_oracle_sdp_codon import ADV, CODON_SDP_SETS, codon_sdp_case, expected

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


def _served(got):
    assert all(alns is not None for alns in got), [i for i, alns in enumerate(got) if alns is None]
    return got


@pytest.mark.parametrize("name", sorted(CODON_SDP_SETS))
def test_device_sdp_matches_reference_vectors(eng, name):
    model, par, recs = codon_sdp_case(name)
    pairs = [(r["query"], r["target"]) for r in recs]
    got = _served(eng.sdp(model, pairs, [r["hsps"] for r in recs], ADV[0], ADV[1], par["dropoff"], par["threshold"], 4))
    total = 0
    for r, alns in zip(recs, got):
        g = [{"score": a.score, "region": list(a.region), "ops": [list(o) for o in a.ops], "vulgar": a.vulgar(r["id"])} for a in alns]
        assert g == expected(r), r["id"]
        total += len(g)
    assert total >= 10


@pytest.mark.parametrize("k", sc.BANDS + ("small",))
def test_device_sdp_on_the_strip_edge_bands(eng, k):
    """One batch per (parameter point, dropoff) of the band."""
    threshold = 10 if k == "small" else sc.THRESHOLD
    groups = {}
    for point, dropoff, pair in sc.band_runs(k):
        groups.setdefault((point, dropoff), []).append(pair)
    for (point, dropoff), pairs in sorted(groups.items()):
        model = sc.model_at(point)
        hsps = [sc.hsps_of(model.params, p) for p in pairs]
        got = _served(eng.sdp(model, [(p["q"], p["t"]) for p in pairs], hsps, 3, 3, dropoff, threshold, 4))
        for p, h, alns in zip(pairs, hsps, got):
            exp = sc.oracle_sdp(model, p["q"], p["t"], h, (3, 3), dropoff, threshold)
            assert [a.as_dict() for a in alns] == exp, (k, point, dropoff, p["kind"], p["row"], p["mirrored"])
            assert exp


@pytest.mark.parametrize("seed", range(4))
def test_device_sdp_fuzz_against_oracle(eng, seed):
    n = 0
    for cs in sc.fuzz_cases(seed):
        model, adv = cs["model"], cs["adv"]
        got = _served(eng.sdp(model, cs["pairs"], cs["hsps"], adv[0], adv[1], cs["dropoff"], cs["threshold"], 4))
        for (q, t), h, alns in zip(cs["pairs"], cs["hsps"], got):
            exp = sc.oracle_sdp(model, q, t, h, adv, cs["dropoff"], cs["threshold"])
            assert [a.as_dict() for a in alns] == exp, (seed, cs["point"], adv, cs["dropoff"], cs["threshold"], len(q), len(t), len(h))
            n += len(exp)
    assert n >= 2


def _strip_batch():
    """Queries of one to five strips (Q + 1 = 40 ... 300 rows) with codon HSPs, and one pair without any."""
    rng = random.Random(4242)
    model = sc.model_at("default")
    pairs, hsps = [], []
    for qmax in (39, 100, 180, 250, 299, 120, 60, 299):
        while True:
            q, t = sc.fuzz_pair(rng, qmax)
            h = sc._codon_hsps(model.params, q, t)
            if h and len(q) > qmax - 30:
                break
        pairs.append((q, t)); hsps.append(h)
    pairs.insert(3, ("ACGTACGTACGTAAA", "TTTTTTGGGGGGCCCCCC")); hsps.insert(3, [])
    return model, pairs, hsps


def test_batch_of_one_to_five_strips_with_an_empty_pair(eng):
    model, pairs, hsps = _strip_batch()
    assert {(len(q) + 1 + 63) // 64 for q, _ in pairs} >= {1, 2, 3, 4, 5}
    got = _served(eng.sdp(model, pairs, hsps, 3, 3, 50, 40, 4))
    assert got[3] == []
    n = 0
    for (q, t), h, alns in zip(pairs, hsps, got):
        if h:
            exp = sc.oracle_sdp(model, q, t, h, (3, 3), 50, 40)
            assert [a.as_dict() for a in alns] == exp, (len(q), len(t), len(h))
            n += len(exp)
    assert n >= 6


def test_arena_too_small_for_some_pairs(eng, monkeypatch):
    """C4GPU_SDP_ARENA_MB (a test hook): 24 chunks of 64 KB for eight pairs that need four to eight each -- the pairs whose
    streams did not fit run again with eight times the arena and are served."""
    model, pairs, hsps = _strip_batch()
    monkeypatch.setenv("C4GPU_SDP_ARENA_MB", "1.5")
    ex.Engine.sdp_stats(reset=True)
    got = _served(eng.sdp(model, pairs, hsps, 3, 3, 50, 40, 4))
    stats = ex.Engine.sdp_stats(reset=True)
    assert stats["reruns"] > 0 and stats["unserved"] == 0, stats
    for (q, t), h, alns in zip(pairs, hsps, got):
        if h:
            assert [a.as_dict() for a in alns] == sc.oracle_sdp(model, q, t, h, (3, 3), 50, 40), (len(q), len(t))


@pytest.mark.parametrize("mt", ["ner", "ungapped:trans"])
def test_models_without_device_passes_still_refuse(eng, mt):
    model = ex.Model(mt)
    with pytest.raises(ex.C4GpuError, match="no device passes"):
        eng.sdp(model, [("ACGTACGTACGTACGT", "ACGTACGTACGTACGT")], [[[0, 0, 4, 20, 2]]], 1, 1, 50, 10, 4)
