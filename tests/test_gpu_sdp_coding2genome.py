"""coding2genome's SDP on the device (c4gpu_sdp_batch: both Scheduler passes of the boundary flavour as sparse wavefronts whose
lanes exchange up to three query rows per step, with their shadow words, c4_sdp_wave.h) through Engine.sdp: against the
reference's own SDP alignments (the four sets of tests/golden/sdp_coding2genome*.jsonl, split codons and strip edges included), on
a batch that mixes one to five strips with a pair without HSPs (expected values from a live refdump --cmd sdp), with an arena too
small for some pairs, and from codon HSPs (advances 3/3) as well as DNA HSPs (1/1).  A pair that comes back unserved (None) is
a failure here."""
import json
import os
import random
import subprocess

import pytest

import exonerate_amd as ex
import coding2genome_cases as cg
import oracle_lib
import sdp_c2g_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDUMP = os.path.join(ROOT, "oracle", "_ref", "refdump")
needs_refdump = pytest.mark.skipif(not os.path.exists(REFDUMP), reason="oracle/_ref/refdump is built by build() where the reference tree is")
WORDLEN = 10
ARENA_MB = "3"                          # C4GPU_SDP_ARENA_MB of test_arena_too_small_for_some_pairs: 48 chunks


@pytest.fixture(scope="module")
def eng():
    e = ex.Engine(0)
    yield e
    e.close()


def _served(got):
    assert all(alns is not None for alns in got), [i for i, alns in enumerate(got) if alns is None]
    return got


def _dicts(alns, qid):
    return [{"score": a.score, "region": list(a.region), "ops": [list(o) for o in a.ops], "vulgar": a.vulgar(qid)} for a in alns]


@pytest.mark.parametrize("name", sorted(sc.SDP_SETS))
def test_device_sdp_matches_reference_vectors(eng, name):
    model, par, recs = sc.sdp_case(name)
    pairs = [(r["query"], r["target"]) for r in recs]
    got = _served(eng.sdp(model, pairs, [r["hsps"] for r in recs], sc.ADV[0], sc.ADV[1], par["dropoff"], par["threshold"], 4))
    total = 0
    for r, alns in zip(recs, got):
        assert _dicts(alns, r["id"]) == sc.expected(r), r["id"]
        total += len(alns)
    assert total >= 10


# ---- one to five strips, live reference -------------------------------------------------------------------------------
_strip = {}


def strip_batch():
    """Queries of one to five strips (Q + 1 = 40 ... 300 rows), genes with one or two introns of any phase, through refdump --cmd
    sdp once: (model, pairs, HSPs, expected alignments); one pair without any HSP put in at index 3."""
    if not _strip:
        rng = random.Random(5151)
        cases = []
        for k, qlen in enumerate((39, 100, 180, 250, 299, 120, 60, 299)):
            n_aa = qlen // 3
            introns = [(n_aa // 3, k % 3, 40 + 6 * k)] + ([(2 * n_aa // 3, (k + 1) % 3, 70 - 3 * k)] if n_aa >= 40 else [])
            q, t = cg.query_of_length(rng, qlen, introns=introns, sub=0.04)
            hits = sc.word_hits(q, t, WORDLEN)
            assert hits
            cases.append(("sb%d" % k, q, t, ",".join("%d:%d" % h for h in hits)))
        path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "c2g_sdp_strips_%d.tsv" % os.getpid())
        with open(path, "w") as f:
            for c in cases:
                f.write("%s\t%s\t%s\t%s\n" % c)
        out = subprocess.run([REFDUMP, "--cmd", "sdp", "--model", "coding2genome", "--input", path, "--dnawordlen", str(WORDLEN),
                              "--suboptmax", "4", "--suboptthreshold", "40"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        os.unlink(path)
        lines = [json.loads(l) for l in out.stdout.decode().splitlines() if l.startswith("{")]
        par, recs = lines[0]["params"], lines[1:]
        assert par["use_boundary"] == 1 and par["dropoff"] == 50 and len(recs) == len(cases)
        pairs = [(c[1], c[2]) for c in cases]
        hsps = [r["hsps"] for r in recs]
        exp = [sc.expected(r) for r in recs]
        ids = [c[0] for c in cases]
        pairs.insert(3, ("ACGTACGTACGTAAA", "TTTTTTGGGGGGCCCCCC")); hsps.insert(3, []); exp.insert(3, []); ids.insert(3, "none")
        _strip["v"] = (sc.sdp_case("sdp_coding2genome")[0], pairs, hsps, exp, ids)
    return _strip["v"]


def _check_strip_batch(eng):
    model, pairs, hsps, exp, ids = strip_batch()
    assert {(len(q) + 1 + 63) // 64 for q, _ in pairs} >= {1, 2, 3, 4, 5}
    got = _served(eng.sdp(model, pairs, hsps, 1, 1, 50, 40, 4))
    assert got[3] == []
    n = introns = 0
    for qid, alns, e in zip(ids, got, exp):
        assert _dicts(alns, qid) == e, qid
        n += len(e)
        introns += sum(len(sc.intron_phases(model, a)) for a in e)
    assert n >= 6 and introns >= 6


@needs_refdump
def test_batch_of_one_to_five_strips_with_an_empty_pair(eng):
    _check_strip_batch(eng)


@needs_refdump
def test_arena_too_small_for_some_pairs(eng, monkeypatch):
    """C4GPU_SDP_ARENA_MB (a test hook): 48 chunks of 64 KB for eight pairs that need 5 to 51 each and 225 in all (counted with
    the simulated passes, tests/sdp_c2g_sim.hip) -- the pairs whose streams did not fit run again with eight times the arena,
    which holds them all, and are served."""
    monkeypatch.setenv("C4GPU_SDP_ARENA_MB", ARENA_MB)
    ex.Engine.sdp_stats(reset=True)
    _check_strip_batch(eng)
    stats = ex.Engine.sdp_stats(reset=True)
    assert stats["reruns"] > 0 and stats["unserved"] == 0, stats



# ---- codon HSPs -------------------------------------------------------------------------------------------------------
def test_codon_hsps_and_dna_hsps_on_one_sets_pairs(eng):
    """SDP takes an HSP as a seed point and a score (sdp.c:438-477, 79-108), whatever set it came from.  The DNA HSPs (advances
    1/1) are grown here by the oracle's HSPset from the pair's word hits and must be the record's; the codon HSPs (3/3) are HSPs
    of the comparison's codon set shape -- same centre-of-best-segment point, same score, advances of three -- so the reference's
    recorded alignments are the expectation for both."""
    model, par, recs = sc.sdp_case("sdp_coding2genome")
    recs = [r for r in recs if r["alignments"]][:16]
    dna, codon = [], []
    for r in recs:
        q, t = r["query"], r["target"]
        h = oracle_lib.hsp_set(model.params, "dna2dna", q.encode(), t.encode(), WORDLEN, 30, par["hsp_threshold"], sc.word_hits(q, t, WORDLEN))
        assert h == r["hsps"], r["id"]
        dna.append(h)
        ch = []
        for qs, ts, length, score, cobs in h:
            c = min(qs + cobs, ts + cobs) // 3
            ch.append([qs + cobs - 3 * c, ts + cobs - 3 * c, c + 1, score, c])
        codon.append(ch)
    pairs = [(r["query"], r["target"]) for r in recs]
    for hsps, adv in ((dna, (1, 1)), (codon, (3, 3))):
        got = _served(eng.sdp(model, pairs, hsps, adv[0], adv[1], par["dropoff"], par["threshold"], 4))
        for r, alns in zip(recs, got):
            assert _dicts(alns, r["id"]) == sc.expected(r), (adv, r["id"])


@pytest.mark.parametrize("mt", ["ner", "ungapped:trans"])
def test_models_without_device_passes_still_refuse(eng, mt):
    model = ex.Model(mt)
    with pytest.raises(ex.C4GpuError, match="no device passes"):
        eng.sdp(model, [("ACGTACGTACGTACGT", "ACGTACGTACGTACGT")], [[[0, 0, 4, 20, 2]]], 1, 1, 50, 10, 4)
