"""Cases and the yardstick of c4gpu_seed_extend_opt (the one-call seeder for soft-masked sets and --seedrepeat > 1).  No tests here.

`replay_opt` is HSPset_seed_hsp (hspset.c:933-997) over a walk's calls with everything the options add: the diagonal tag and the
counter of --seedrepeat (:950-970), the horizon test, the two-stage extension of a soft-masked set with a dropped seed's masked end
as its entry's horizon (:981-995).  It stands on Scorer / seed_hsp of tests/test_hsp_softmask.py and the codon scorer of
tests/hsp_codon_cases.py and shares no code with the library.  tests/test_seed_fused_opt_cases.py pins it on seed_fused_cases.replay,
on test_hsp_softmask.seed_set and on the reference binary's recorded output before anything is held to it."""
import math
import random

import seed_fused_cases as sf
import codon_seed_cases as cs
from codon_cases import CODONS, AA
from hsp_codon_cases import CodonScorer
from test_hsp_softmask import Scorer, seed_hsp, masked_view

ADVANCE = {"dna2dna": (1, 1), "protein2protein": (1, 1), "protein2dna": (1, 3), "codon2codon": (3, 3)}


def scorer(params, match, query, target, mask_query=False, mask_target=False):
    if match == "codon2codon":
        return CodonScorer(params, query, target, mask_query, mask_target)
    return Scorer(params, match, query, target, mask_query, mask_target)


def entry_of(match, qlen, qs, ts):
    """(section, query frame, target frame) of a seed, or None for a seed without an entry (query advance 1: C's truncating
    remainder of a negative sum; the codon set takes the sum as a guint and always has one), hspset.c:935-943."""
    aq, at = ADVANCE[match]
    total = ts * aq - qs * at + qlen
    if aq == 3:
        return ((total & 0xffffffff) % qlen, qs % aq, ts % at)
    section = int(math.fmod(total, qlen))
    return None if section < 0 else (section, 0, ts % at)


def replay_opt(params, match, queries, target, calls, seedlen, dropoff, threshold, mask_query=False, mask_target=False,
               seed_repeat=1, tagless=False, detail=None):
    """calls: [query, query_start, target_start] in walk order.  Returns ([(walk index, query, [qs, ts, length, score, cobs])] of
    the kept HSPs, {"n_hits", "n_extended", "n_below", "n_kept"}): n_extended counts the extensions that ran, n_below those of them
    that stored nothing (below the threshold, or dropped after the forbidding round).  tagless: a per-entry counter WITHOUT the
    diagonal tag (what the reference does not do).  detail: receives {"verdict": per call 0 not extended / 1 extended, nothing
    stored / 2 kept, "dropped": walk indices of the dropped seeds}."""
    aq, at = ADVANCE[match]
    if seed_repeat < 1:
        raise ValueError("seed_repeat below 1")
    if seed_repeat > 1 and match == "protein2dna":
        raise ValueError("no parity target: the reference leaves its horizon array there")
    scorers = [scorer(params, match, q, target, mask_query, mask_target) for q in queries]
    entries, kept, verdict, dropped_at = {}, [], [], []
    n_extended = 0
    for k, (qi, qs, ts) in enumerate(calls):
        sc = scorers[qi]
        key = entry_of(match, sc.qlen, qs, ts)
        e = entries.setdefault((qi,) + key, [0, 0, 0]) if key is not None else [0, 0, 0]     # horizon, counter, tag
        if seed_repeat > 1:
            tag = (ts * aq - qs * at + sc.qlen) & 0xffffffff
            if e[2] != tag and not tagless:
                e[0], e[1], e[2] = 0, 0, tag
        if ts < e[0]:
            verdict.append(0)
            continue
        if seed_repeat > 1:
            e[1] += 1
            if e[1] < seed_repeat:
                verdict.append(0)
                continue
            e[1] = 0
        h, dropped = seed_hsp(sc, seedlen, dropoff, threshold, qs, ts)
        n_extended += 1
        e[0] = h[1] + h[2] * at
        if not dropped and h[3] >= threshold:
            kept.append((k, qi, h))
            verdict.append(2)
        else:
            verdict.append(1)
            if dropped:
                dropped_at.append(k)
    if detail is not None:
        detail["verdict"], detail["dropped"] = verdict, dropped_at
    return kept, dict(n_hits=len(calls), n_extended=n_extended, n_below=n_extended - len(kept), n_kept=len(kept))


def protein_symbols(target):
    return bytes(sf.PROTEIN_COLUMN.get(c, 0) for c in target)


class Case:
    """One pair list against one target as Engine.seed_extend takes it under the options: the residues WITH their case in the
    pairs, the scan strings and the word table from the masked views (Sequence_mask: a masked symbol becomes the wildcard, which
    is column 0), and the walk's calls for replay_opt."""

    def __init__(self, name, match, queries, target, wordlen, dropoff, threshold, mask_query=False, mask_target=False, seed_repeat=1):
        self.name, self.match, self.queries, self.target = name, match, queries, target
        self.wordlen = self.seedlen = wordlen
        self.dropoff, self.threshold = dropoff, threshold
        self.mask_query, self.mask_target, self.seed_repeat = mask_query, mask_target, seed_repeat
        qwild = "X" if match in ("protein2protein", "protein2dna") else "N"
        twild = "X" if match == "protein2protein" else "N"
        qs = [masked_view(q, qwild, mask_query) for q in queries]
        t = masked_view(target, twild, mask_target)
        if match == "dna2dna":
            self.width = 5
            self.words, self.emits = sf.word_table(qs, wordlen, sf.DNA_COLUMN, self.width)
            self.strings, self.tpos_scale, self.tpos_offset, self.tpos_modifier = [sf.dna_symbols(t)], 1, [0], wordlen - 1
        elif match == "protein2protein":
            self.width = len(AA) + 1
            self.words, self.emits = sf.word_table(qs, wordlen, sf.PROTEIN_COLUMN, self.width)
            self.strings, self.tpos_scale, self.tpos_offset, self.tpos_modifier = [protein_symbols(t)], 1, [0], wordlen - 1
        else:
            self.width = len(AA) + 1
            if match == "protein2dna":
                self.words, self.emits = sf.word_table(qs, wordlen, sf.PROTEIN_COLUMN, self.width)
            else:
                self.words, self.emits = cs.word_table(qs, wordlen)
            self.strings, self.tpos_scale, self.tpos_offset, self.tpos_modifier = sf.frame_symbols(t), 3, [0, 1, 2], wordlen * 3 - 3
        self.calls = sf.walk(self.width, wordlen, self.words, self.emits, self.strings, self.tpos_scale, self.tpos_offset,
                             self.tpos_modifier)
        self.pairs = [(q, target) for q in queries]

    def replay(self, params, detail=None, **over):
        opt = dict(mask_query=self.mask_query, mask_target=self.mask_target, seed_repeat=self.seed_repeat)
        opt.update(over)
        return replay_opt(params, self.match, self.queries, self.target, self.calls, self.seedlen, self.dropoff, self.threshold,
                          detail=detail, **opt)

    def run(self, eng, params, cap=None, **over):
        opt = dict(mask_query=self.mask_query, mask_target=self.mask_target, seed_repeat=self.seed_repeat)
        opt.update(over)
        return eng.seed_extend(params, self.match, self.pairs, self.width, self.wordlen, self.words, self.emits, self.strings,
                               self.tpos_scale, self.tpos_offset, self.tpos_modifier, self.seedlen, self.dropoff, self.threshold,
                               cap=cap, **opt)


def _dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _other(rng, c, alphabet="ACGT"):
    return rng.choice([x for x in alphabet if x != c])


def _lower(s, a, b):
    return s[:a] + s[a:b].lower() + s[b:]


def case_dropped_then_extended():
    """A 60-nt query and its copy in the target behind 7 other bases.  Copy positions 14..30 are lower case.  The scan meets the
    words of the first 14 bases (three of them), then the words from 31 on.  With --softmasktarget the first seed stops in front
    of position 14 with 14 * 5 = 70 < 75: DROPPED, its entry's horizon the masked end, 7 + 14.  The seed at copy position 31 lies
    past it and is extended (29 * 5 = 145 after the forbidding round, then freely over the whole copy).  Under the plain rule, on
    the same scan strings, the first seed grows over the whole copy and the seed at 31 is skipped."""
    rng = random.Random(1201)
    q = _dna(rng, 60)
    t = "".join(_other(rng, c) for c in q[:7]) + _lower(q, 14, 31) + _dna(rng, 5)
    return Case("dropped_then_extended", "dna2dna", [q], t, 12, 30, 75, mask_target=True)


def case_masked_keeps_fewer():
    """Two 50-nt queries.  The target holds a lower-case copy of each; 13 bases of the first copy are upper case (an island of two
    words, 65 < 75 after the forbidding round: dropped), 30 of the second (kept).  Unmasked, both copies are kept."""
    rng = random.Random(1202)
    qa, qb = _dna(rng, 50), _dna(rng, 50)
    ca, cb = qa.lower(), qb.lower()
    ca = ca[:20] + ca[20:33].upper() + ca[33:]
    cb = cb[:10] + cb[10:40].upper() + cb[40:]
    t = _dna(rng, 9) + ca + _dna(rng, 11) + cb + _dna(rng, 4)
    return Case("masked_keeps_fewer", "dna2dna", [qa, qb], t, 12, 30, 75, mask_target=True)


def _single_copies(rng, q, spots, alphabet, filler_len):
    """A target of filler with q[p:p + n] at position `at` for every (p, n, at) of `spots`, each copy with a mismatch on either
    side (against the query's own neighbours on that diagonal), so that it gives exactly n - w + 1 word hits."""
    t = [rng.choice(alphabet) for _ in range(filler_len)]
    for p, n, at in spots:
        t[at:at + n] = q[p:p + n]
        if p > 0 and at > 0:
            t[at - 1] = _other(rng, q[p - 1], alphabet)
        if p + n < len(q) and at + n < len(t):
            t[at + n] = _other(rng, q[p + n], alphabet)
    return "".join(t)


def case_tag(seed_repeat=2):
    """A 100-nt query; one 12-mer of it at target position 30 and the same 12-mer at 130: two single word hits one query length
    apart, on two diagonals that share a horizon entry.  Under --seedrepeat 2 the second hit finds another diagonal's tag, clears
    the counter and is held back like the first: nothing is kept.  A counter without the tag reaches 2 and extends the second."""
    rng = random.Random(1203)
    q = _dna(rng, 100)
    t = _single_copies(rng, q, [(40, 12, 30), (40, 12, 130)], "ACGT", 200)
    return Case("tag", "dna2dna", [q], t, 12, 30, 40, seed_repeat=seed_repeat)


def case_counters(match, seed_repeat):
    """Copies of exactly w, w + 1 and w + 2 symbols of three queries (1, 2 and 3 word hits on a diagonal of their own): repeat 2
    keeps the last two, repeat 3 the last."""
    rng = random.Random(1204 + len(match))
    if match == "dna2dna":
        alphabet, w, qlen, thr, dropoff = "ACGT", 12, 90, 40, 30
    else:
        alphabet, w, qlen, thr, dropoff = AA, 6, 60, 12, 20
    queries = ["".join(rng.choice(alphabet) for _ in range(qlen)) for _ in range(3)]
    t = []
    for k, q in enumerate(queries):
        t.append(_single_copies(rng, q, [(20, w + k, 25)], alphabet, 70))
    return Case("counters_%s_%d" % (match, seed_repeat), match, queries, "".join(t), w, dropoff, thr, seed_repeat=seed_repeat)


def _orf(rng, n):
    return "".join(rng.choice(CODONS[rng.choice(AA)]) for _ in range(n))


def case_codon_wrapped_shared_entry(seed_repeat=2):
    """A translated query of 30 codons (90 nt).  The target opens with the word q[63:75] at 0 (3 * (0 - 63) + 90 < 0: wrapped) and
    holds q[51:63] at 18 (3 * (18 - 51) + 90 < 0: wrapped too); the sums are 90 apart, so in unsigned arithmetic both land on one
    entry, in the same frames.  One word hit each: under --seedrepeat 2 the tag holds both back; a tagless counter extends the
    second."""
    rng = random.Random(1205)
    while True:
        q = _orf(rng, 30)
        t = q[63:75] + "TAATAA" + q[51:63] + "TAA"
        c = Case("codon_wrapped_shared_entry", "codon2codon", [q], t, 4, 20, 10, seed_repeat=seed_repeat)
        if [x[1:] for x in c.calls] == [[63, 0], [51, 18]]:
            return c


def case_mask_at_the_ends():
    """The query's copy IS the target; first and last residue of both are lower case, both sides flagged.  The masked positions are
    the first and the last byte of either sequence: the forbidding round stops inside them, the free round takes them in."""
    rng = random.Random(1206)
    q = _dna(rng, 61)
    q = q[0].lower() + q[1:-1] + q[-1].lower()
    return Case("mask_at_the_ends", "dna2dna", [q], q, 12, 30, 75, mask_query=True, mask_target=True)


def case_one_lower_base(match):
    """protein2dna: a 30-residue query against its codons, ONE base (the middle one of codon 12) lower case, target flagged.
    codon2codon: the same ORF on both sides, the one lower-case base in the QUERY, query flagged.  The codon with the base is
    masked as a whole: no word crosses it, the forbidding round stops at it from both sides."""
    rng = random.Random(1207)
    pep = "".join(rng.choice(AA) for _ in range(30))
    dna = "".join(rng.choice(CODONS[a]) for a in pep)
    low = dna[:37] + dna[37].lower() + dna[38:]
    if match == "protein2dna":
        return Case("one_lower_base_protein2dna", match, [pep], low, 6, 20, 30, mask_target=True)
    return Case("one_lower_base_codon2codon", match, [low], dna, 4, 20, 30, mask_query=True)


def case_edge_opt(name, seed_repeat=1):
    """EDGE_SHAPES of seed_fused_cases.py (targets of 2 047 to 4 097 symbols, one to three radix passes) with lower-case stretches
    planted over the target, one of them across the 2 048-symbol edge where there is one: --softmasktarget, or --seedrepeat 2."""
    c = sf.case_edge(name)
    t = c.target
    mask_target = seed_repeat == 1
    if mask_target:
        # the planted pieces of seed_fused_cases._planted start at 5, at len - 70 and (where the target has that edge) at 2 023: 13
        # bases of each stay upper case (65 < 75 after the forbidding round), the 16 behind them are masked; a few stretches more
        rng = random.Random(1300 + len(name))
        for at in [5, len(t) - 70] + ([2048 - 25] if len(t) > 2048 + 40 else []):
            t = _lower(t, at + 13, at + 29)
        for _ in range(6):
            at = rng.randrange(100, len(t) - 100)
            t = _lower(t, at, at + rng.randint(8, 30))
    return Case(name + ("_masked" if mask_target else "_repeat%d" % seed_repeat), "dna2dna", c.queries, t, 12, 30, 75,
                mask_target=mask_target, seed_repeat=seed_repeat)


def record_case(par, rec, masked=True, seed_repeat=1):
    """A recorded pair (hsp_softmask_*, hsp_seedrepeat_*) as a Case."""
    return Case(rec["id"], par["match"], [rec["query"]], rec["target"], par["seedlen"], par["dropoff"], par["threshold"],
                mask_query=masked and par.get("mask_query", False), mask_target=masked and par.get("mask_target", False),
                seed_repeat=seed_repeat)
