"""HSP seeding of the translated models (Match_Type_CODON2CODON, src/comparison/match.c:508-539: ungapped:trans and
coding2coding).  No tests here.

A Python restatement for the codon match beside the one of tests/test_hsp_softmask.py, whose extension and single-seed routines
it reuses unchanged (they take the advances from the scorer): both sequences are scored as "row of the codon starting here",
both advances are 3, either side's soft mask ORs the three bases of a codon (Match_3_mask_func, match.c:212-220; wildcard 'n'),
and the horizon entry of a seed is keyed as the reference computes it -- Sequence.len is a guint (sequence.h:83), so
hspset.c:942-943 takes (diag + qlen) % qlen in 32-bit UNSIGNED arithmetic and a seed with 3 * (qs - ts) > qlen lands on an
entry another diagonal owns.  tests/test_hsp_codon.py holds it to the reference's recorded codon sets
(tests/golden/hsp_codon*.jsonl, tools/make_codon_hsp_golden.py)."""
from golden_util import load_set
from test_hsp_softmask import seed_hsp

CODON_SETS = ["hsp_codon", "hsp_codon_softmask"]


class CodonScorer:
    """What one codon-vs-codon HSP position scores and when it is masked; the interface of test_hsp_softmask.Scorer."""
    aq = at = 3

    def __init__(self, params, query, target, mask_query=False, mask_target=False):
        idx, nt2d, trans, aa = bytes(params.submat_index), bytes(params.nt2d), bytes(params.trans), bytes(params.aa)
        self.mat = [[params.protein_submat[a][b] for b in range(24)] for a in range(24)]
        rows = lambda s: [idx[aa[trans[nt2d[s[x]] | (nt2d[s[x + 1]] << 4) | (nt2d[s[x + 2]] << 8)]]] for x in range(len(s) - 2)]
        low = lambda c: 97 <= c <= 122 and c != 110
        mask = lambda s: [low(s[x]) or low(s[x + 1]) or low(s[x + 2]) for x in range(len(s) - 2)]
        q, t = query.encode(), target.encode()
        self.qlen, self.tlen = len(q), len(t)
        self.qrow, self.trow = rows(q), rows(t)
        self.qmask = mask(q) if mask_query else None
        self.tmask = mask(t) if mask_target else None
        self.masking = bool(mask_query or mask_target)

    def score(self, qp, tp):
        return self.mat[self.qrow[qp]][self.trow[tp]]

    def masked(self, qp, tp):
        return bool((self.qmask and self.qmask[qp]) or (self.tmask and self.tmask[tp]))


def entry(qlen, qs, ts):
    """The horizon entry (section, query frame, target frame) of a codon seed, hspset.c:935-943 in the reference's unsigned
    arithmetic."""
    return (((ts * 3 - qs * 3 + qlen) & 0xffffffff) % qlen, qs % 3, ts % 3)


def wrapped(qlen, qs, ts):
    """Is the sum negative as a signed number: the seed's section is the remainder of a number near 2^32."""
    return ts * 3 - qs * 3 + qlen < 0


def seed_set(sc, seedlen, dropoff, threshold, seeds):
    """HSPset_seed_hsp over a whole scan (seed_repeat 1): per seed None (under its horizon) or (hsp, dropped), and the list of
    HSPs stored (score >= threshold: HSP_store)."""
    horizon, per_seed, kept = {}, [], []
    for qs, ts in seeds:
        key = entry(sc.qlen, qs, ts)
        if ts < horizon.get(key, 0):
            per_seed.append(None)
            continue
        h, dropped = seed_hsp(sc, seedlen, dropoff, threshold, qs, ts)
        per_seed.append((h, dropped))
        horizon[key] = h[1] + h[2] * 3
        if not dropped and h[3] >= threshold:
            kept.append(h)
    return per_seed, kept


def load_codon_set(name):
    """(params, records) of a codon golden file.  A record: id, query, target, mask_query, mask_target, seeds, `single` (per
    seed the reference's own answer on a fresh set: [query_start, target_start, length, score, cobs], or None for a seed that
    stores nothing -- below the threshold, or dropped), `dropped_end` (per seed None, or the masked end a dropped seed leaves in
    its horizon entry) and `set` (what the set held after the whole scan)."""
    recs = load_set(name)
    return recs[0]["params"], recs[1:]
