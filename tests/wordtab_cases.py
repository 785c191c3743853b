"""Edge inputs for the word-table build, in column space with score tables of their own (tests/test_wordtab_model.py shows on the
model that each has the property it is there for; tests/test_gpu_wordtab_build.py holds the device to the model on them).
A case: name, width, wordlen, strings, sources, scores, threshold, use_dropoff, and a string to scan."""
import random

import wordtab_model as wm


class Case:
    def __init__(self, name, width, wordlen, strings, sources=None, scores=None, threshold=0, use_dropoff=True, scan=None):
        self.name, self.width, self.wordlen = name, width, wordlen
        self.strings = [bytes(s) for s in strings]
        self.sources = list(sources) if sources is not None else [(k, 1, 0) for k in range(len(self.strings))]
        self.scores, self.threshold, self.use_dropoff = scores, threshold, use_dropoff
        self.scan = bytes(scan) if scan is not None else b"\0".join(self.strings)

    def args(self):
        return (self.width, self.wordlen, self.strings, self.sources, self.scores, self.threshold, self.use_dropoff)

    def model(self):
        return wm.build(*self.args())


def flat(width, diag, off):
    return [[(diag if a == b else off) if a and b else 0 for b in range(width)] for a in range(width)]


def rand_string(rng, n, width, lo=1):
    return bytes(rng.randint(lo, width - 1) for _ in range(n))


def empties():
    """Nothing to build from: each gives zero words, and a scan of anything gives no hits."""
    s = flat(5, 5, -4)
    scan = bytes([1, 2, 3, 4, 1, 2, 3, 4, 4, 3, 2, 1])
    return [Case("no_string", 5, 4, [], scores=s, threshold=9, scan=scan),
            Case("empty_string", 5, 4, [b""], scores=s, threshold=9, scan=scan),
            Case("shorter_than_a_word", 5, 4, [bytes([1, 2, 3]), bytes([4]), b""], scores=s, threshold=9, scan=scan),
            Case("all_columns_zero", 5, 4, [bytes(9)], scores=s, threshold=9, scan=scan),
            Case("resets_too_close", 5, 4, [bytes([1, 2, 3, 0, 4, 1, 2, 0, 3, 3, 3])], scores=s, threshold=9, scan=scan)]


def wordlen_one():
    # one letter a word: the neighbourhood is a row of the table (no two-letter prefix to deal out)
    s = [[0, 0, 0, 0, 0], [0, 4, 2, -1, -3], [0, 2, 5, 0, -2], [0, -1, 0, 6, 3], [0, -3, -2, 3, 7]]
    return Case("wordlen_1", 5, 1, [bytes([1, 3, 0, 3]), bytes([4])], scores=s, threshold=3)


def identical_queries():
    q = bytes([1, 2, 3, 4, 1, 2, 3, 4, 2])                       # (1,2,3,4) twice in each query
    return Case("two_identical_queries", 5, 4, [q, q])


def neighbour_across_queries():
    # query 0 spells (1,2,3,4), query 1 spells (1,2,3,3): one mismatch = 9 = the limit, each is in the other's neighbourhood
    return Case("neighbour_across_queries", 5, 4, [bytes([1, 2, 3, 4]), bytes([1, 2, 3, 3])], scores=flat(5, 5, -4), threshold=9)


def all_neighbours():
    """width 6, wordlen 3, every score 1: every word is every other word's neighbour.  All 125 words are spelt, so each table word
    has 124 sources (more than a wave's 64 lanes) and the links, 125 * 124 = 15 500, fill more than seven sort tiles."""
    words = [bytes([a, b, c]) for a in range(1, 6) for b in range(1, 6) for c in range(1, 6)]
    random.Random(5).shuffle(words)
    half = len(words) // 2
    return Case("all_neighbours", 6, 3, [b"\0".join(words[:half]), b"\0".join(words[half:])], scores=flat(6, 1, 1), threshold=0,
                scan=bytes([1, 2, 3, 4, 5, 5, 1]))


def many_links():
    """DNA-like: 300 letters, words of 6, one mismatch allowed: 18 neighbours a word, more than 2 * 2048 links."""
    rng = random.Random(11)
    return Case("many_links", 5, 6, [rand_string(rng, 150, 5), rand_string(rng, 150, 5)], scores=flat(5, 5, -4), threshold=9)


def wide_codes():
    """width 25, wordlen 7: the codes of words that start with column 18 or above are >= 2^32 (18 * 25^6 = 4 394 531 250)."""
    rng = random.Random(13)
    s = flat(25, 5, -4)
    for a, b in ((24, 23), (20, 2), (3, 19)):
        s[a][b] = s[b][a] = 1
    strings = [rand_string(rng, 14, 25, lo=18), rand_string(rng, 12, 25), bytes([24, 23, 24, 23, 24, 23, 24, 1])]
    return Case("wide_codes", 25, 7, strings, scores=s, threshold=9)


def prefix_failure():
    """s[1][2] = 6 > s[1][1] = 2.  For W = (3,1,3) and N = (2,2,3): the first letter loses 3 > the limit 2, so the walk never
    enters it, yet the whole word scores -1 + 6 + 2 = 7 against a bar of 6 - 2 = 4.  The rule is on prefixes (wordhood.c:283)."""
    s = flat(4, 2, -1)
    s[1][2] = 6
    return Case("prefix_failure", 4, 3, [bytes([3, 1, 3, 1, 1, 2]), bytes([2, 1, 2])], scores=s, threshold=2)


def absolute_threshold():
    """--useworddropoff no: the limit is a score, not a loss.  s[a][a] = a, s[a][b] = (a + b) // 2, but s[1][5] = 7: the word
    (1,1,1) scores 3 against itself, under the limit 8 -- the walk does not reach the word itself -- while (5,1,1) scores 9."""
    s = [[0] * 6 for _ in range(6)]
    for a in range(1, 6):
        for b in range(1, 6):
            s[a][b] = a if a == b else (a + b) // 2
    s[1][5] = 7
    return Case("absolute_threshold", 6, 3, [bytes([1, 1, 1, 4, 5, 2]), bytes([3, 3, 3, 3])], scores=s, threshold=8, use_dropoff=False)


def translated_frames():
    """Three frame strings of one pair: scale 3, offsets 0 / 1 / 2 (seeder.c:540-541)."""
    rng = random.Random(17)
    f = [rand_string(rng, 12, 23), rand_string(rng, 12, 23), rand_string(rng, 11, 23)]
    f[1] = f[1][:3] + f[0][2:6] + f[1][7:]                        # frames that share a word
    return Case("translated_frames", 23, 4, f, sources=[(0, 3, 0), (0, 3, 1), (0, 3, 2)], scores=flat(23, 5, -4), threshold=9)


def edges():
    return [wordlen_one(), identical_queries(), neighbour_across_queries(), all_neighbours(), many_links(), wide_codes(),
            prefix_failure(), absolute_threshold(), translated_frames()]


def scan_hits(case, table):
    """What c4gpu_seed_scan reports for case.scan on `table` (wordtab_model.build's form): (position, emission index)."""
    at = {c: (table["emit_first"][k], table["emit_first"][k + 1]) for k, c in enumerate(table["codes"])}
    out, run = [], 0
    for i, c in enumerate(case.scan):
        run = run + 1 if c else 0
        if run >= case.wordlen:
            lo, hi = at.get(wm.code_of(case.width, case.scan[i - case.wordlen + 1:i + 1]), (0, 0))
            out += [(i, e) for e in range(lo, hi)]
    return out
