"""c4gpu_seed_extend with codon emissions (C4GPU_MATCH_CODON2CODON: a translated query against a translated target) against
codon_seed_cases.replay -- HSPset_seed_hsp restated with the horizon entry in the reference's unsigned arithmetic, pinned on the
reference's recorded codon sets in tests/test_hsp_codon.py: the recorded scans themselves, and generated cases with three frame
strings at scale 3, three queries in one table, 2 047, 2 048 and 2 049 word hits (the sort tile and the verdict block hold 2 048)
over more than one count block per frame, wrapped seeds among them; the capacity protocol; the first hits; the refusals."""
import pytest

import exonerate_amd as ex
import codon_seed_cases as cs
import hsp_codon_cases as hc

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
def par():
    return hc.load_codon_set("hsp_codon")[0]


@pytest.fixture(scope="module")
def sized(params, par):
    """The generated cases and their replays, made once."""
    out = {}
    for n in (2047, 2048, 2049):
        c = cs.case_hits(n, par["seedlen"], par["dropoff"], par["threshold"])
        out[n] = (c, c.replay(params))
    return out


def test_recorded_scans(eng, params, par):
    """Every recorded scan, handed over in the recorded order.  The seeder of a codon set walks the target's nucleotides once
    (its automaton spells the words in bases), so the scan is position-ascending: a table with one one-symbol word per target
    position that has seeds (its emissions: that position's seeds in order), one string that holds word w's symbol at that
    position, scale 1.  The kept list is what the reference's set held."""
    for rec in hc.load_codon_set("hsp_codon")[1]:
        seeds = [tuple(s) for s in rec["seeds"]]
        assert seeds == sorted(seeds, key=lambda s: s[1]), rec["id"]
        words, emits, sym = [], [], bytearray(len(rec["target"]))
        for ts in sorted({s[1] for s in seeds}):
            group = [s for s in seeds if s[1] == ts]
            words.append((len(words) + 1, len(group)))
            emits += [(0, qs) for qs, _ in group]
            sym[ts] = len(words)
        assert len(words) < 255
        got, stats = eng.seed_extend(params, "codon2codon", [(rec["query"], rec["target"])], 255, 1, words, emits, [bytes(sym)], 1, [0],
                                     0, par["seedlen"], par["dropoff"], par["threshold"])
        exp, exp_stats = cs.replay(params, [rec["query"]], rec["target"], [[0, qs, ts] for qs, ts in seeds], par["seedlen"],
                                   par["dropoff"], par["threshold"])
        assert (got, stats) == (exp, exp_stats), rec["id"]
        assert [h for _, _, h in got] == rec["set"], rec["id"]


@pytest.mark.parametrize("n_hits", [2047, 2048, 2049])
def test_generated_cases(eng, params, sized, n_hits):
    c, (exp, exp_stats) = sized[n_hits]
    assert exp_stats["n_hits"] == n_hits and len(c.strings) == 3 and c.tpos_scale == 3 and min(len(s) for s in c.strings) > 2048
    assert {(qs % 3, ts % 3) for _, qs, ts in c.calls} == {(a, b) for a in range(3) for b in range(3)}
    assert sum(hc.wrapped(len(c.queries[qi]), qs, ts) for qi, qs, ts in c.calls) >= 10
    first = []
    got, stats = c.run(eng, params, first_hits=first)
    assert stats == exp_stats
    assert got == exp                                     # (the walk index runs frame-major over the three frame strings)
    assert stats["n_kept"] >= 10 and stats["n_below"] > 0 and stats["n_extended"] < n_hits
    want = [-1] * len(c.queries)
    for k, (qi, _, _) in enumerate(c.calls):
        if want[qi] < 0:
            want[qi] = k
    assert first == want


def test_capacity(eng, params, sized):
    c, (exp, exp_stats) = sized[2049]
    got, stats = c.run(eng, params, cap=exp_stats["n_kept"] - 1)
    assert got == [] and stats == exp_stats                # nothing written, the counters say how much room is needed
    got, stats = c.run(eng, params, cap=stats["n_kept"])
    assert got == exp and stats == exp_stats
    got, stats = c.run(eng, params, cap=0)
    assert got == [] and stats == exp_stats


def test_refusals(eng, params, sized):
    c = sized[2047][0]

    def call(match="codon2codon", emits=c.emits, seedlen=c.seedlen):
        return eng.seed_extend(params, match, c.pairs, c.width, c.wordlen, c.words, emits, c.strings, 3, [0, 1, 2], c.tpos_modifier,
                               seedlen, c.dropoff, c.threshold)

    with pytest.raises(ex.C4GpuError, match="unknown match type"):
        call(match=7)
    with pytest.raises(ex.C4GpuError, match="unknown match type"):
        call(match=4)
    # the seed bound counts the query advance: query_pos + seedlen * 3 <= qlen.  The last word of a query's frame starts
    # wordlen codons from the end, so one codon more no longer fits -- with advance 1 it would
    with pytest.raises(ex.C4GpuError, match="inside its pair"):
        call(seedlen=c.seedlen + 1)
    assert call()[1] == sized[2047][1][1]                  # the context serves the case afterwards
