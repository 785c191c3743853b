"""Cases and the yardstick of c4gpu_seed_extend for C4GPU_MATCH_CODON2CODON (a translated query against a translated target).
No tests here.

`replay` is built as seed_fused_cases.replay is -- HSPset_seed_hsp restated seed by seed over the walk's calls, a horizon
dictionary, the entry moved to the HSP's target end whether or not the HSP reaches the threshold -- around the codon restatement
of hsp_codon_cases.py (the oracle has no codon-vs-codon HSP), with the entry keyed in the reference's unsigned arithmetic: every
seed has one.  tests/test_hsp_codon.py pins it on the reference's recorded codon sets.  The word table of a translated query holds
the words of its three frames, every emission a NUCLEOTIDE position (seeder.c:540-545); the target is walked frame by frame."""
import random

import seed_fused_cases as sf
from codon_cases import CODONS, AA
from hsp_codon_cases import CodonScorer, entry
from test_hsp_softmask import seed_hsp


def replay(params, queries, target, calls, seedlen, dropoff, threshold):
    """calls: [query, query_start, target_start] in walk order -> ([(walk index, query, hsp)] of the kept HSPs, the counters)."""
    scorers = [CodonScorer(params, q, target) for q in queries]
    horizon, kept = {}, []
    n_extended = n_below = 0
    for k, (qi, qs, ts) in enumerate(calls):
        key = (qi,) + entry(scorers[qi].qlen, qs, ts)
        if ts < horizon.get(key, 0):
            continue
        h, _ = seed_hsp(scorers[qi], seedlen, dropoff, threshold, qs, ts)
        n_extended += 1
        horizon[key] = h[1] + h[2] * 3
        if h[3] >= threshold:
            kept.append((k, qi, h))
        else:
            n_below += 1
    return kept, dict(n_hits=len(calls), n_extended=n_extended, n_below=n_below, n_kept=len(kept))


def word_table(queries, wordlen):
    """Exact words of the queries' three frames: ([(code, emissions)], [(query, nucleotide position)]), words in order of first
    appearance."""
    width = len(AA) + 1
    table, order = {}, []
    for qi, q in enumerate(queries):
        for f in range(3):
            cols = [sf.PROTEIN_COLUMN.get(sf.CODON_AA.get(q[p:p + 3], "*"), 0) for p in range(f, len(q) - 2, 3)]
            for k in range(len(cols) - wordlen + 1):
                w = cols[k:k + wordlen]
                if 0 in w:
                    continue
                code = 0
                for c in w:
                    code = code * width + c
                if code not in table:
                    table[code] = []
                    order.append(code)
                table[code].append((qi, f + 3 * k))
    return [(code, len(table[code])) for code in order], [e for code in order for e in table[code]]


class Case:
    """Everything Engine.seed_extend takes for codon emissions, and the walk's calls for `replay`: three frame strings, scale 3."""
    match = "codon2codon"

    def __init__(self, queries, target, wordlen, dropoff, threshold):
        self.queries, self.target = queries, target
        self.wordlen = self.seedlen = wordlen
        self.dropoff, self.threshold = dropoff, threshold
        self.width = len(AA) + 1
        self.strings, self.tpos_scale, self.tpos_offset, self.tpos_modifier = sf.frame_symbols(target), 3, [0, 1, 2], wordlen * 3 - 3
        self.words, self.emits = word_table(queries, wordlen)
        self.calls = sf.walk(self.width, wordlen, self.words, self.emits, self.strings, 3, self.tpos_offset, self.tpos_modifier)
        self.pairs = [(q, target) for q in queries]

    def replay(self, params):
        return replay(params, self.queries, self.target, self.calls, self.seedlen, self.dropoff, self.threshold)

    def run(self, eng, params, cap=None, first_hits=None):
        return eng.seed_extend(params, self.match, self.pairs, self.width, self.wordlen, self.words, self.emits, self.strings,
                               self.tpos_scale, self.tpos_offset, self.tpos_modifier, self.seedlen, self.dropoff, self.threshold,
                               cap=cap, first_hits=first_hits)


def _orf(rng, n):
    return "".join(rng.choice(CODONS[rng.choice(AA)]) for _ in range(n))


def case_hits(n_hits, wordlen, dropoff, threshold):
    """Three queries (99, 100 and 101 codons behind flanks of 0, 1 and 2 bases: every query frame) and one target of mutated
    copies of their pieces at every offset modulo 3, the end of the first query at the target's start (wrapped seeds), over more
    than the 2 048 symbols of a count block per frame -- then single words of a fourth query planted behind stop codons, one word
    hit each, until the walk has exactly `n_hits` hits."""
    rng = random.Random(909)
    queries = ["" + _orf(rng, 99), "G" + _orf(rng, 100), "CA" + _orf(rng, 101), _orf(rng, 300)]
    parts = []
    for k in range(13):
        q = queries[k % 3]
        n = rng.randint(50, 80) * 3 if k else 150
        at = (len(q) - n) if k == 0 else rng.randrange(0, len(q) - n)
        piece = list(q[at:at + n])
        for x in rng.sample(range(n), 3):
            piece[x] = rng.choice([c for c in "ACGT" if c != piece[x]])
        parts.append("".join(piece) + "TAA" + "T" * (k % 3))
    target = "".join(parts)
    target += _orf(rng, max(0, (3 * 2100 - len(target)) // 3 + 1)) + "TAA"
    case = Case(queries, target, wordlen, dropoff, threshold)
    have = len(case.calls)
    assert have <= n_hits, (have, n_hits)
    filler, step = queries[3], 0
    while have < n_hits:                                        # one more single-hit word, then count again
        word = filler[step * wordlen * 3:(step + 1) * wordlen * 3]
        assert len(word) == wordlen * 3, "the filler query has no words left"
        grown = Case(queries, target + word + "TAA", wordlen, dropoff, threshold)
        if len(grown.calls) <= n_hits:
            target, case, have = grown.target, grown, len(grown.calls)
        step += 1
    assert len(case.calls) == n_hits
    return case
