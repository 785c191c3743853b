"""c4gpu_seed_extend (word scan to stored HSPs in one device call, the hits staying on the device) against
seed_fused_cases.replay -- HSPset_seed_hsp restated around the oracle's extension, pinned on the oracle's own sets in
tests/test_seed_fused_cases.py -- over every reference-generated seeder record and the generated cases; its capacity protocol and
every refusal; and, at a size the oracle is too slow for, against the device's existing calls (seed_scan, chain numbers as the
drop-in's hsp_flush computes them, hsp_extend_chains, threshold)."""
import pytest

import exonerate_amd as ex
import seed_fused_cases as sf
from test_oracle_seed import SEED_SETS, load_seed_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def params():
    return ex.default_params()


def _record(eng, params, rec, point):
    dropoff, threshold = sf.points(rec["match"])[point]
    words, emits = sf.record_table(rec)
    pairs = [(q, rec["target"]) for q in rec["queries"]]
    got = eng.seed_extend(params, rec["match"], pairs, rec["width"], rec["wordlen"], words, emits, [bytes(rec["symbols"])], 1, [0],
                          rec["tpos_modifier"], rec["wordlen"], dropoff, threshold)
    exp = sf.replay(params, rec["match"], rec["queries"], rec["target"], rec["expected"], rec["wordlen"], dropoff, threshold)
    return got, exp


@pytest.mark.parametrize("point", ["default", "low"])
@pytest.mark.parametrize("name", SEED_SETS)
def test_records(eng, params, name, point):
    """Kept HSPs, their walk indices and pairs, and all four counters, record by record."""
    for rec in load_seed_set(name):
        (got, stats), (exp, exp_stats) = _record(eng, params, rec, point)
        assert stats == exp_stats, rec["id"]
        assert got == exp, rec["id"]
        assert stats["n_kept"] > 0 and stats["n_extended"] < stats["n_hits"]


GENERATED = {"one_diagonal_two_hsps": sf.case_one_diagonal_two_hsps,
             "shared_entry_across_diagonals": sf.case_shared_entry_across_diagonals,        # three frame strings, scale 3
             "negative_section": sf.case_negative_section}
GENERATED.update({s[0]: (lambda n=s[0]: sf.case_edge(n)) for s in sf.EDGE_SHAPES})


@pytest.mark.parametrize("name", sorted(GENERATED))
def test_generated_cases(eng, params, name):
    c = GENERATED[name]()
    exp, exp_stats = c.replay(params)
    got, stats = c.run(eng, params)
    assert stats == exp_stats
    assert got == exp                                     # (the walk index runs frame-major over the three frame strings)
    assert stats["n_kept"] > 0


def test_nothing_to_report(eng, params):
    for c in sf.cases_nothing_to_report():
        got, stats = c.run(eng, params)
        assert got == [] and stats == dict(n_hits=0, n_extended=0, n_below=0, n_kept=0), c.name


def test_capacity(eng, params):
    c = sf.case_edge("edge_2049_65535")
    exp, exp_stats = c.replay(params)
    assert exp_stats["n_kept"] >= 5
    got, stats = c.run(eng, params, cap=exp_stats["n_kept"] - 1)
    assert got == [] and stats == exp_stats                # nothing written, the counters say how much room is needed
    got, stats = c.run(eng, params, cap=stats["n_kept"])
    assert got == exp and stats == exp_stats


def test_refusals(eng, params):
    """Every refusal of the header, each with its message; the context serves a record afterwards."""
    c = sf.case_one_diagonal_two_hsps()
    q, t = c.queries[0], c.target

    def call(match=c.match, pairs=c.pairs, words=c.words, emits=c.emits, strings=c.strings):
        return eng.seed_extend(params, match, pairs, c.width, c.wordlen, words, emits, strings, 1, [0], c.tpos_modifier, c.seedlen,
                               c.dropoff, c.threshold)

    assert call()[1]["n_kept"] == 2
    with pytest.raises(ex.C4GpuError, match="unknown match type"):
        call(match=7)
    with pytest.raises(ex.C4GpuError, match="no emissions set"):
        call(emits=None)
    with pytest.raises(ex.C4GpuError, match="emissions, %d given" % (len(c.emits) - 1)):
        call(emits=c.emits[:-1])
    with pytest.raises(ex.C4GpuError, match="pair outside"):
        call(emits=[(1, p) for _, p in c.emits])
    with pytest.raises(ex.C4GpuError, match="negative pair or query position"):
        call(emits=[(0, -1)] + c.emits[1:])
    with pytest.raises(ex.C4GpuError, match="negative pair or query position"):
        call(emits=[(-1, 0)] + c.emits[1:])
    with pytest.raises(ex.C4GpuError, match="one target buffer"):
        call(pairs=[(q, t), (q, t + "A")], emits=c.emits)
    with pytest.raises(ex.C4GpuError, match="one target buffer"):
        call(pairs=[(q, t), (q, t[:-1] + "A")], emits=c.emits)            # the same length in another buffer
    with pytest.raises(ex.C4GpuError, match="inside its pair"):             # found on the device: the seed would end past the query
        call(emits=[(0, len(q) - 3)] + c.emits[1:])
    with pytest.raises(ex.C4GpuError, match="alphabet"):
        call(pairs=[(q[:30] + "!" + q[31:], t)])
    # horizon entries: three pairs of one 240 Mb protein against DNA are 3 * 3 * 240e6 > 2^31 - 1 (refused before anything is read)
    big = bytes(240 * 1000 * 1000)
    with pytest.raises(ex.C4GpuError, match="horizon entries"):
        eng.seed_extend(params, "protein2dna", [(big, t)] * 3, c.width, c.wordlen, c.words, c.emits, c.strings, 3, [0], 15, 6, 20, 12)
    del big
    # word hits: one word with 2^18 emissions at 8 203 positions is 2 150 367 232 > 2^31 - 1 (counted, never written)
    with pytest.raises(ex.C4GpuError, match="word hits"):
        eng.seed_extend(params, "dna2dna", [("A" * 40, "A" * 8214)], 5, 12, [(sum(5 ** k for k in range(12)), 1 << 18)],
                        [(0, 0)] * (1 << 18), [bytes([1]) * 8214], 1, [0], 11, 12, 30, 75)
    rec = load_seed_set(SEED_SETS[0])[0]
    (got, stats), (exp, exp_stats) = _record(eng, params, rec, "default")
    assert got == exp and stats == exp_stats


def test_against_the_existing_calls_at_size(eng, params):
    """64 queries of about 1 kb with planted homologies against a 200 kb target: seed_scan, the chain numbers of the drop-in's
    hsp_flush (one per (set, section, target frame) in order of first use; a seed without an entry a chain of its own that
    nothing skips), hsp_extend_chains and the threshold give what seed_extend gives.  (Both are the device; the old route is
    pinned in tests/test_gpu_seed.py and tests/test_gpu_hsp.py.)"""
    c = sf.case_at_size()
    hits, _ = eng.seed_scan(c.width, c.wordlen, c.words, c.strings[0])
    seeds, chain, horizon0, slot = [], [], [], {}
    for pos, e in hits:
        qi, qs = c.emits[e]
        ts = pos - c.tpos_modifier
        qlen = len(c.queries[qi])
        section = (ts - qs + qlen) % qlen if ts - qs + qlen >= 0 else -1
        if section < 0:
            chain.append(len(horizon0))
            horizon0.append(-2 ** 31)
        else:
            if (qi, section) not in slot:
                slot[(qi, section)] = len(horizon0)
                horizon0.append(0)
            chain.append(slot[(qi, section)])
        seeds.append((qi, qs, ts))
    assert len(seeds) > 2000
    old = eng.hsp_extend_chains(params, c.match, c.pairs, c.seedlen, c.dropoff, seeds, chain, horizon0)
    exp = [(k, seeds[k][0], h) for k, h in enumerate(old) if h[2] >= 0 and h[3] >= c.threshold]
    n_ext = sum(h[2] >= 0 for h in old)
    got, stats = c.run(eng, params)
    assert got == exp and len(exp) >= 100
    assert stats == dict(n_hits=len(seeds), n_extended=n_ext, n_below=n_ext - len(exp), n_kept=len(exp))


@pytest.mark.parametrize("name", ["edge_4097_65537", "edge_2048_257", "shared_entry_across_diagonals"])
def test_first_hits(eng, params, name):
    """c4gpu_seed_extend_first_hits: per pair the walk index of its first word hit, kept or not (the order the reference
    creates and reports its Comparisons in); -1 for a pair without hits."""
    c = GENERATED[name]()
    first = []
    got, stats = eng.seed_extend(params, c.match, c.pairs, c.width, c.wordlen, c.words, c.emits, c.strings, c.tpos_scale, c.tpos_offset,
                                 c.tpos_modifier, c.seedlen, c.dropoff, c.threshold, first_hits=first)
    exp = [-1] * len(c.queries)
    for k, (qi, _, _) in enumerate(c.calls):
        if exp[qi] < 0:
            exp[qi] = k
    assert first == exp and max(exp) >= 0
    if len(c.queries) > 2:                                 # 64 queries: some have no hit at all
        assert -1 in exp and len({x for x in exp if x >= 0}) > 5
