"""HSP seeding of soft-masked sequences (--softmaskquery / --softmasktarget): a Python restatement of HSPset_seed_hsp
(src/comparison/hspset.c:933-997) with both extension stages (:981-995, HSP_extend :748-815) and the diagonal horizon,
independent of the library's kernels.  It is held first to the reference's own per-seed and whole-set HSPs with masks off
(tests/golden/hsp_*.jsonl, refdump --cmd hsp), then to what the reference BINARY printed for soft-masked inputs
(tests/golden/hsp_softmask_*.jsonl, tools/make_golden.py: exonerate -m ungapped --showsugar yes, each input with and without
the softmask options).  The device entry points are held to this restatement in test_gpu_hsp_softmask.py."""
import pytest

from golden_util import load_set
from test_oracle_hsp import HSP_SETS

SOFTMASK_SETS = ["hsp_softmask_dna2dna_t", "hsp_softmask_dna2dna_q", "hsp_softmask_dna2dna_qt",
                 "hsp_softmask_protein2protein_t", "hsp_softmask_protein2protein_q",
                 "hsp_softmask_protein2dna_t", "hsp_softmask_protein2dna_qt"]
ADVANCE = {"dna2dna": (1, 1), "protein2protein": (1, 1), "protein2dna": (1, 3)}


class Scorer:
    """What one HSP position scores (Match_1_1_*_score_func, Match_1_3 via Translate_base: match.c) and when it is masked
    (match.c:156-158,178-182,212-220; alphabet.h:87 with the SOFTMASK filters of alphabet.c:124-129: every lower-case
    letter but the wildcard itself, 'n' / 'x', which both filters send to the same symbol)."""

    def __init__(self, params, match, query, target, mask_query=False, mask_target=False):
        self.aq, self.at = ADVANCE[match]
        idx = bytes(params.submat_index)
        mat = params.dna_submat if match == "dna2dna" else params.protein_submat
        mat = [[mat[a][b] for b in range(24)] for a in range(24)]
        q, t = query.encode(), target.encode()
        self.qlen, self.tlen = len(q), len(t)
        self.qrow = [idx[c] for c in q]
        if match == "protein2dna":
            nt2d, trans, aa = bytes(params.nt2d), bytes(params.trans), bytes(params.aa)
            self.trow = [idx[aa[trans[nt2d[t[x]] | (nt2d[t[x + 1]] << 4) | (nt2d[t[x + 2]] << 8)]]] for x in range(len(t) - 2)]
        else:
            self.trow = [idx[c] for c in t]
        self.mat = mat
        low = lambda c, wild: 97 <= c <= 122 and c != wild
        qw = ord("n") if match == "dna2dna" else ord("x")
        tw = ord("x") if match == "protein2protein" else ord("n")
        self.qmask = [low(c, qw) for c in q] if mask_query else None
        if not mask_target:
            self.tmask = None
        elif self.at == 3:
            self.tmask = [low(t[x], tw) or low(t[x + 1], tw) or low(t[x + 2], tw) for x in range(len(t) - 2)]
        else:
            self.tmask = [low(c, tw) for c in t]
        self.masking = bool(mask_query or mask_target)

    def score(self, qp, tp):
        return self.mat[self.qrow[qp]][self.trow[tp]]

    def masked(self, qp, tp):
        return bool((self.qmask and self.qmask[qp]) or (self.tmask and self.tmask[tp]))


def extend(sc, h, dropoff, forbid):
    """HSP_extend (hspset.c:748-815) on h = [query_start, target_start, length, score]."""
    aq, at = sc.aq, sc.at
    qs, ts, length, score = h
    maxscore = score
    qp, tp, ext, maxext = qs - aq, ts - at, 1, 0
    while qp >= 0 and tp >= 0:
        if forbid and sc.masked(qp, tp):
            break
        score += sc.score(qp, tp)
        if maxscore <= score:
            maxscore, maxext = score, ext
        elif score < 0 or maxscore - score >= dropoff:
            break
        qp -= aq; tp -= at; ext += 1
    qp, tp = qs + length * aq, ts + length * at
    qs -= maxext * aq; ts -= maxext * at; length += maxext
    score, ext, maxext = maxscore, 1, 0
    while qp + aq <= sc.qlen and tp + at <= sc.tlen:
        if forbid and sc.masked(qp, tp):
            break
        score += sc.score(qp, tp)
        if maxscore <= score:
            maxscore, maxext = score, ext
        elif score < 0 or maxscore - score >= dropoff:
            break
        qp += aq; tp += at; ext += 1
    return [qs, ts, length + maxext, maxscore]


def seed_hsp(sc, seedlen, dropoff, threshold, qs, ts):
    """One seed past its horizon test: ([query_start, target_start, length, score, cobs], dropped).  Dropped (only with a
    soft-masked side): the masked-extended nascent HSP, cobs 0 (hspset.c:985-989).  Without masking the threshold is
    HSP_store's business (:893), not decided here."""
    aq, at = sc.aq, sc.at
    length = seedlen
    while length > 0 and sc.score(qs, ts) <= 0:                         # HSP_trim_ends (:850-878)
        qs += aq; ts += at; length -= 1
    while length > 0 and sc.score(qs + (length - 1) * aq, ts + (length - 1) * at) <= 0:
        length -= 1
    h = [qs, ts, length, sum(sc.score(qs + i * aq, ts + i * at) for i in range(length))]      # HSP_init (:725-746)
    if sc.masking:
        h = extend(sc, h, dropoff, True)
        if h[3] < threshold:
            return h + [0], 1
    h = extend(sc, h, dropoff, False)
    run, cobs = 0, h[2]
    for i in range(h[2]):                                                # HSP_find_cobs (:426-441)
        run += sc.score(h[0] + i * aq, h[1] + i * at)
        if run >= (h[3] >> 1):
            cobs = i
            break
    return h + [cobs], 0


def seed_set(sc, seedlen, dropoff, threshold, seeds):
    """HSPset_seed_hsp over a whole scan (seed_repeat 1): per seed None (under its horizon) or (hsp, dropped), and the list
    of HSPs stored (score >= threshold: HSP_store)."""
    horizon, per_seed, kept = {}, [], []
    for qs, ts in seeds:
        key = ((ts * sc.aq - qs * sc.at + sc.qlen) % sc.qlen, qs % sc.aq, ts % sc.at)
        if ts < horizon.get(key, 0):
            per_seed.append(None)
            continue
        h, dropped = seed_hsp(sc, seedlen, dropoff, threshold, qs, ts)
        per_seed.append((h, dropped))
        horizon[key] = h[1] + h[2] * sc.at                               # HSP_target_end, of the masked HSP when dropped
        if not dropped and h[3] >= threshold:
            kept.append(h)
    return per_seed, kept


def masked_view(seq, wild, on):
    """The sequence as the seeder reads it (Alphabet_Filter_Type_MASKED): masked symbols become the wildcard."""
    seq = seq if not on else "".join(wild if (c.islower() and c != wild.lower()) else c for c in seq)
    return seq.upper()


def word_hits(params, par, query, target, mask_query, mask_target):
    """Every shared word of the pair in target-scan order; a word over a masked position matches nothing."""
    match, w = par["match"], par["seedlen"]
    q = masked_view(query, "N" if match == "dna2dna" else "X", mask_query)
    t = masked_view(target, "X" if match == "protein2protein" else "N", mask_target)
    bad = "N" if match == "dna2dna" else "X"
    words = {}
    for i in range(len(q) - w + 1):
        if bad not in q[i:i + w]:
            words.setdefault(q[i:i + w], []).append(i)
    if match == "protein2dna":
        nt2d, trans, aa = bytes(params.nt2d), bytes(params.trans), bytes(params.aa)
        tb = t.encode()
        res = [chr(aa[trans[nt2d[tb[x]] | (nt2d[tb[x + 1]] << 4) | (nt2d[tb[x + 2]] << 8)]]) for x in range(len(tb) - 2)]
        view = lambda j: "".join(res[j + 3 * k] for k in range(w))
        last = len(t) - 3 * w
    else:
        view = lambda j: t[j:j + w]
        last = len(t) - w
    return [(i, j) for j in range(last + 1) for i in words.get(view(j), ())]


@pytest.mark.parametrize("name", HSP_SETS)
def test_restatement_matches_reference_with_masks_off(params, name):
    recs = load_set(name)
    par, recs = recs[0]["params"], recs[1:]
    assert par["seed_repeat"] == 1
    for r in recs:
        sc = Scorer(params, par["match"], r["query"], r["target"])
        for (qs, ts), exp in zip(r["seeds"], r["single"]):
            got, dropped = seed_hsp(sc, par["seedlen"], par["dropoff"], par["threshold"], qs, ts)
            assert not dropped
            if exp is None:
                assert got[3] < par["threshold"], (r["id"], qs, ts)
            else:
                assert got == exp, (r["id"], qs, ts)
        assert seed_set(sc, par["seedlen"], par["dropoff"], par["threshold"], r["seeds"])[1] == r["set"], r["id"]


def test_lower_case_on_an_unflagged_side_is_not_masked(params):
    """Alphabet_is_masked (alphabet.h:87): without the side's softmask option nothing is masked, whatever the case."""
    q, t = "ACGTTGCAAGCTTGACCATG" * 2, "ttgacc" + ("ACGTTGCAAGCTTGACCATG" * 2).lower() + "gatt"
    plain = seed_hsp(Scorer(params, "dna2dna", q, t), 12, 30, 75, 0, 6)
    assert plain == seed_hsp(Scorer(params, "dna2dna", q, t, mask_query=True), 12, 30, 75, 0, 6)
    assert plain[0][:4] == [0, 6, 40, 200] and plain[1] == 0
    assert seed_hsp(Scorer(params, "dna2dna", q, t, mask_target=True), 12, 30, 75, 0, 6) == ([0, 6, 12, 60, 0], 1)


@pytest.mark.parametrize("name", SOFTMASK_SETS)
def test_restatement_finds_what_the_reference_binary_printed(params, name):
    """Fed every shared word of a recorded pair in target-scan order, the restatement must hold every HSP the reference
    printed (same ends, same score) -- with the softmask options and without -- and nothing at all for a pair the reference
    dropped entirely."""
    recs = load_set(name)
    par, recs = recs[0]["params"], recs[1:]
    lost = 0
    for r in recs:
        for mq, mt, key in ((False, False, "plain"), (par["mask_query"], par["mask_target"], "masked")):
            sc = Scorer(params, par["match"], r["query"], r["target"], mq, mt)
            seeds = word_hits(params, par, r["query"], r["target"], mq, mt)
            kept = seed_set(sc, par["seedlen"], par["dropoff"], par["threshold"], seeds)[1]
            mine = {(h[0], h[1], h[2], h[3]) for h in kept}
            for h in r[key]:
                assert tuple(h) in mine, (r["id"], key, h, sorted(mine))
            if not r[key]:
                assert not mine, (r["id"], key, sorted(mine))
        lost += len([h for h in r["plain"] if h not in r["masked"]])
    assert lost >= 6, name                                               # the mask decides (the generator asserts it too)
