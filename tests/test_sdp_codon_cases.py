"""What the strip-edge bands of coding2coding's SDP (tests/sdp_codon_cases.py) claim, decided on the oracle's alignments alone:
every pair takes its event -- a match in one of the three frames, a query frameshift of one or two bases, a codon insert, a
target-side event -- on the row it was built for, on the side of its one seed point that the forward pass (rows u) or the
reverse pass (rows Q - u) finds.  A band that does not show its claim fails here, whatever the device does with it."""
import pytest

import sdp_codon_cases as sc


@pytest.mark.parametrize("k", sc.BANDS)
def test_band_takes_every_event_on_its_row(k):
    b = 64 * k
    claims = set()
    for point, dropoff, pair in sc.band_runs(k):
        model = sc.model_at(point)
        hsps = sc.hsps_of(model.params, pair)
        alns = sc.oracle_sdp(model, pair["q"], pair["t"], hsps, (3, 3), dropoff, sc.THRESHOLD)
        assert alns, (point, dropoff, pair["kind"], pair["row"], pair["mirrored"])
        missing = sc.shows(model, pair, hsps[0], alns)
        assert missing is None, (point, dropoff, missing)
        if dropoff == 5:                                     # nothing but matches lives: the path is the chain from end to end
            assert all(sum(n for _, n in a["ops"]) == a["region"][2] // 3 + 2 for a in alns)
        claims.add((pair["kind"], pair["row"] - b, pair["mirrored"], dropoff, point))
    for mirrored in (False, True):
        for point in sc.POINTS:
            assert {("match", r, mirrored, 50, point) for r in (-3, -2, -1)} <= claims
        assert {("match", r, mirrored, 5, "default") for r in (-3, -2, -1)} <= claims
        assert {("q1", -1, mirrored, 50, "altparams"), ("q2", -2, mirrored, 50, "altparams"), ("qc", -3, mirrored, 50, "altparams")} <= claims
        rows = (-1, 0) + ((-63,) if k >= 2 else ())
        assert {(kind, r, mirrored, 50, "altparams") for kind in ("t1", "t2", "tc") for r in rows} <= claims


@pytest.mark.parametrize("k", sc.BANDS)
def test_band_queries_end_one_to_six_rows_into_the_last_strip(k):
    b = 64 * k
    lengths = {len(pair["q"]) for _, _, pair in sc.band_runs(k)}
    assert lengths == set(range(b - 2, b + 4)), sorted(lengths)
    assert {(len(pair["q"]) + 1) - b for _, _, pair in sc.band_runs(k)} == set(range(-1, 5))      # rows past the edge
    if k >= 2:                                              # homologous through the middle strips: each receives and leaves carried rows
        for _, _, pair in sc.band_runs(k):
            assert len(pair["q"]) >= b - 2


def test_small_band():
    runs = sc.band_runs("small")
    assert {len(p["q"]) for _, _, p in runs} == set(range(3, 9))
    for point, dropoff, pair in runs:
        model = sc.model_at(point)
        hsps = sc.hsps_of(model.params, pair)
        assert hsps[0][2] == 1
        alns = sc.oracle_sdp(model, pair["q"], pair["t"], hsps, (3, 3), dropoff, 10)
        assert alns and alns[0]["region"][2] == 3 * (len(pair["q"]) // 3), (pair["q"], pair["t"], alns)
