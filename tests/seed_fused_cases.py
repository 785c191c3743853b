"""Cases and the yardstick of c4gpu_seed_extend (word scan to stored HSPs in one device call).  No tests here.

`replay` is HSPset_seed_hsp (hspset.c:933-997, seed_repeat 1, no soft mask) restated around the oracle's single-seed extension:
a horizon dictionary per (query, section, target frame) with C's truncating remainder for the section, oracle_lib.hsp_extend for
every seed that is not skipped, the entry moved to the HSP's target end whether or not the HSP reaches the threshold.
tests/test_seed_fused_cases.py pins it on oracle_lib.hsp_set over every reference-generated seeder record.  The generators build
the cases no record holds; their word hits come from a dictionary walk in Python (`walk`), in Seeder_add_target's order."""
import math
import random

import exonerate_amd as ex
import oracle_lib
from golden_util import load_set
from codon_cases import CODONS, AA

DNA_COLUMN = {c: i + 1 for i, c in enumerate("ACGT")}                  # automaton columns of the generated cases; 0: outside
PROTEIN_COLUMN = {c: i + 1 for i, c in enumerate(AA)}
CODON_AA = {c: a for a, cs in CODONS.items() for c in cs}


def points(match):
    """(seedlen is the record's wordlen) -> {"default": (dropoff, threshold), "low": (dropoff, threshold)} of a seeder record's
    match type: hsp_<match>.jsonl, and the lowered set (hsp_dna2dna_low; for protein the values of hsp_protein2dna_drop)."""
    par = lambda name: load_set(name)[0]["params"]
    low = par("hsp_dna2dna_low" if match == "dna2dna" else "hsp_protein2dna_drop")
    dflt = par("hsp_" + match)
    return {"default": (dflt["dropoff"], dflt["threshold"]), "low": (low["dropoff"], low["threshold"])}


def replay(params, match, queries, target, calls, seedlen, dropoff, threshold, key="section", detail=None):
    """calls: [query, query_start, target_start] in walk order.  Returns ([(walk index, query, [qs, ts, length, score, cobs])]
    of the kept HSPs, {"n_hits", "n_extended", "n_below", "n_kept"}).  key="diagonal" keys the horizon by the raw diagonal
    instead of its section (what the reference does NOT do).  detail: a dict that receives {"entry_kept": {entry: kept HSPs}}."""
    at = 3 if match == "protein2dna" else 1
    t = target if isinstance(target, bytes) else target.encode()
    qs_b = [q if isinstance(q, bytes) else q.encode() for q in queries]
    horizon, kept, entry_kept = {}, [], {}
    n_extended = n_below = 0
    for k, (qi, qs, ts) in enumerate(calls):
        qlen = len(qs_b[qi])
        diag = ts - qs * at
        section = int(math.fmod(diag + qlen, qlen))                   # C's %: negative for a negative dividend
        entry = None
        if section >= 0:
            entry = (qi, section if key == "section" else diag, ts % at)
            if ts < horizon.get(entry, 0):
                continue
        h = oracle_lib.hsp_extend(params, match, qs_b[qi], t, seedlen, dropoff, qs, ts)
        n_extended += 1
        if entry is not None:
            horizon[entry] = h[1] + h[2] * at
        if h[3] >= threshold:
            kept.append((k, qi, h))
            if entry is not None:
                entry_kept[entry] = entry_kept.get(entry, 0) + 1
        else:
            n_below += 1
    if detail is not None:
        detail["entry_kept"] = entry_kept
    return kept, dict(n_hits=len(calls), n_extended=n_extended, n_below=n_below, n_kept=len(kept))


def record_table(rec):
    """A seeder record's word table as the drop-in builds it (tests/test_gpu_seed.py): words = [(code, emissions)],
    emits = [(query, query position)] -- a word's own seeds, then the seeds of each neighbour word."""
    words, emits = [], []
    for code, own, nbrs in rec["words"]:
        mine = list(own)
        for v in nbrs:
            mine += rec["words"][v][1]
        words.append((code, len(mine)))
        emits += [tuple(e) for e in mine]
    return words, emits


def word_table(queries, wordlen, column, width):
    """Exact words of the queries: ([(code, emissions)], [(query, query position)]), words in order of first appearance."""
    table, order = {}, []
    for qi, q in enumerate(queries):
        for p in range(len(q) - wordlen + 1):
            cols = [column.get(c, 0) for c in q[p:p + wordlen]]
            if 0 in cols:
                continue
            code = 0
            for c in cols:
                code = code * width + c
            if code not in table:
                table[code] = []
                order.append(code)
            table[code].append((qi, p))
    words = [(code, len(table[code])) for code in order]
    emits = [e for code in order for e in table[code]]
    return words, emits


def walk(width, wordlen, words, emits, strings, tpos_scale, tpos_offset, tpos_modifier):
    """Seeder_add_target's calls over the symbol strings, string after string: [query, query_start, target_start]."""
    first, table = 0, {}
    for code, n in words:
        table[code] = (first, n)
        first += n
    calls = []
    for s, sym in enumerate(strings):
        for i in range(wordlen - 1, len(sym)):
            w = sym[i - wordlen + 1:i + 1]
            if 0 in w:
                continue
            code = 0
            for c in w:
                code = code * width + c
            if code in table:
                f, n = table[code]
                for e in range(f, f + n):
                    calls.append([emits[e][0], emits[e][1], i * tpos_scale + tpos_offset[s] - tpos_modifier])
    return calls


def dna_symbols(target):
    return bytes(DNA_COLUMN.get(c, 0) for c in target)


def frame_symbols(target):
    """The three translated frames of a DNA target as protein automaton columns (stop codons and anything else: 0)."""
    out = []
    for f in range(3):
        out.append(bytes(PROTEIN_COLUMN.get(CODON_AA.get(target[p:p + 3], "*"), 0) for p in range(f, len(target) - 2, 3)))
    return out


class Case:
    """One generated case: everything Engine.seed_extend takes, and the walk's calls for `replay`."""

    def __init__(self, name, match, queries, target, wordlen, dropoff, threshold):
        self.name, self.match, self.queries, self.target = name, match, queries, target
        self.wordlen = self.seedlen = wordlen
        self.dropoff, self.threshold = dropoff, threshold
        if match == "dna2dna":
            self.width, column = 5, DNA_COLUMN
            self.strings, self.tpos_scale, self.tpos_offset, self.tpos_modifier = [dna_symbols(target)], 1, [0], wordlen - 1
        else:
            assert match == "protein2dna"
            self.width, column = len(AA) + 1, PROTEIN_COLUMN
            self.strings, self.tpos_scale, self.tpos_offset, self.tpos_modifier = frame_symbols(target), 3, [0, 1, 2], wordlen * 3 - 3
        self.words, self.emits = word_table(queries, wordlen, column, self.width)
        self.calls = walk(self.width, wordlen, self.words, self.emits, self.strings, self.tpos_scale, self.tpos_offset,
                          self.tpos_modifier)
        self.pairs = [(q, target) for q in queries]

    def replay(self, params, key="section", detail=None):
        return replay(params, self.match, self.queries, self.target, self.calls, self.seedlen, self.dropoff, self.threshold, key,
                      detail)

    def run(self, eng, params, cap=None):
        return eng.seed_extend(params, self.match, self.pairs, self.width, self.wordlen, self.words, self.emits, self.strings,
                               self.tpos_scale, self.tpos_offset, self.tpos_modifier, self.seedlen, self.dropoff, self.threshold,
                               cap=cap)


def _dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _other(rng, c):
    return rng.choice([x for x in "ACGT" if x != c])


def case_one_diagonal_two_hsps():
    """(a) A 60-nt query; the target is the query with its 15 middle bases replaced by mismatches: 22 and 23 matching bases
    (+5 each) around 15 mismatches (-4 each: 60 below the best, over the dropoff of 30) -- two HSPs on one diagonal."""
    rng = random.Random(101)
    q = _dna(rng, 60)
    t = q[:22] + "".join(_other(rng, c) for c in q[22:37]) + q[37:]
    return Case("one_diagonal_two_hsps", "dna2dna", [q], t, 12, 30, 75)


def case_shared_entry_across_diagonals():
    """(b) Protein against DNA: qlen = 30 residues with Q[20:30] == Q[10:20]; the target codes Q and then Q[10:30].  The repeat
    puts seeds on the diagonals 30 bases either side of the main one, and 30 bases are one query length in RESIDUES: those
    diagonals share the main diagonal's horizon entry (section 0), so the reference skips seeds a per-diagonal key extends."""
    rng = random.Random(202)
    rep = "".join(rng.choice(AA) for _ in range(10))
    q = "".join(rng.choice(AA) for _ in range(10)) + rep + rep
    code = lambda pep: "".join(rng.choice(CODONS[a]) for a in pep)
    t = code(q) + code(q[10:30])
    return Case("shared_entry_across_diagonals", "protein2dna", [q], t, 6, 20, 12)


def case_negative_section():
    """(c) The codons of Q[20:26] of a 30-residue query at target offset 3: diag = 3 - 60, diag + qlen = -27 -- C's remainder is
    negative, the seed has no horizon entry and is always extended."""
    rng = random.Random(303)
    q = "".join(rng.choice(AA) for _ in range(30))
    t = _dna(rng, 3) + "".join(rng.choice(CODONS[a]) for a in q[20:26]) + _dna(rng, 30)
    return Case("negative_section", "protein2dna", [q], t, 6, 20, 12)


def _planted(rng, name, query_lens, target_len, n_plants):
    """DNA queries of the given lengths; a random target with pieces of the queries (40-60 nt, one mismatch inside) planted over
    it: one from the first query, one from the last, one across the 2 048-symbol edge of a count block where the target has one,
    the rest anywhere."""
    queries = [_dna(rng, n) for n in query_lens]
    t = list(_dna(rng, target_len))
    spots = [5, target_len - 70]
    if target_len > 2048 + 40:
        spots.append(2048 - 25)
    step = max(80, target_len // (n_plants + 1))
    x = 90
    while len(spots) < n_plants and x + 70 < target_len - 80:
        if all(abs(x - s) >= 75 for s in spots):
            spots.append(x)
        x += step
    assert len(spots) >= n_plants, (name, spots)
    for k, at in enumerate(spots):
        qi = 0 if k == 0 else (len(queries) - 1 if k == 1 else rng.randrange(len(queries)))
        q = queries[qi]
        n = min(rng.randint(40, 60), len(q))
        p = rng.randrange(len(q) - n + 1)
        piece = list(q[p:p + n])
        piece[n // 2] = _other(rng, piece[n // 2])
        t[at:at + n] = piece
    return Case(name, "dna2dna", queries, "".join(t)[:target_len], 12, 30, 75)


# (d) targets around the 2 048 symbols of a count block; sum of qlen * at = horizon entries around 2^8 and 2^16, so the slot
# numbers (0 .. entries, the last one for seeds without an entry) need one, two, two and three radix passes
EDGE_SHAPES = [("edge_2047_255", 2047, [128, 127]), ("edge_2048_257", 2048, [128, 129]),
               ("edge_2049_65535", 2049, [1024] * 63 + [1023]), ("edge_4097_65537", 4097, [1024] * 63 + [1025])]


def case_edge(name):
    for k, (nm, tlen, qlens) in enumerate(EDGE_SHAPES):
        if nm == name:
            return _planted(random.Random(400 + k), nm, qlens, tlen, 8)
    raise KeyError(name)


def cases_nothing_to_report():
    """(e) A target shorter than a word, a target of only column 0, a table no word of which occurs."""
    rng = random.Random(505)
    q = _dna(rng, 50)
    return [Case("short_target", "dna2dna", [q], q[:11], 12, 30, 75),
            Case("column0_target", "dna2dna", [q], "N" * 300, 12, 30, 75),
            Case("no_word_occurs", "dna2dna", ["AC" * 30], "GT" * 200, 12, 30, 75)]


def case_at_size():
    """64 queries of about 1 kb with planted homologies against a 200 kb target (the device's two routes against each other)."""
    rng = random.Random(606)
    return _planted(rng, "at_size", [rng.randint(900, 1100) for _ in range(64)], 200000, 120)


def default_params():
    return ex.default_params()
