"""The seeder's word table in plain Python: what Seeder_add_query leaves in the reference's automaton, as closed rules
(c4gpu_wordtab_build in include/c4gpu.h states them; exonerate_amd/csrc/c4_wordtab_build.inc computes them on the device).

    occurrences   position i of a string ends a word when its last `wordlen` columns are non-zero (seeder.c:499-519); the word
                  starts at pos = i - wordlen + 1, its seed is (pair, pos * pos_scale + pos_offset) (seeder.c:540-545);
                  numbered g = 0, 1, ... string by string, position ascending
    own(c)        the seeds of code c's occurrences, g descending (prepended: seeder.c:103-107)
    hood(W)       walked once, at W's first seed (seeder.c:546-553): the pruned depth-first walk of wordhood.c:192-218,277-299
    emissions(N)  own(N), then own(W) for every W with N in hood(W), first(W) descending (prepended: seeder.c:121-124)

Slow on purpose: the neighbourhood is the reference's walk letter by letter, nothing is hashed or sorted cleverly.  Also here:
the column maps of the reference's two automata and the score tables in column space, so that a golden record's queries can be
fed to the model (and to the device) as the reference fed them to its automaton."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the comparison alphabets (alphabet.c:182,191)
MEMBERS = {"dna2dna": "ACGT", "protein2protein": "ARNDCQEGHILKMFPSTWYUV*"}
# flags -> (word limit, use_dropoff, wordlen): the defaults of hspset.c:31-76
DEFAULTS = {"dna2dna": {"wordlen": 12, "limit": 0}, "protein2protein": {"wordlen": 6, "limit": 4}}


def hood(width, wordlen, word, scores, threshold, use_dropoff):
    """The words WordHood_traverse reaches from `word` (a tuple of columns), the word itself included if the walk reaches it:
    a node at depth d is entered only if the score of its d + 1 letters is >= depth_threshold[d] (wordhood.c:283)."""
    self_score = [scores[c][c] for c in word]
    t = sum(self_score) - threshold if use_dropoff else threshold            # wordhood.c:331-337
    thr = [0] * wordlen                                                      # wordhood.c:207-216
    thr[wordlen - 1] = t
    for i in range(wordlen - 2, -1, -1):
        thr[i] = thr[i + 1] - self_score[i + 1]
    out = []

    def walk(d, score, prefix):
        for c in range(1, width):
            s = score + scores[word[d]][c]
            if s < thr[d]:
                continue
            if d == wordlen - 1:
                out.append(prefix + (c,))
            else:
                walk(d + 1, s, prefix + (c,))
    walk(0, 0, ())
    return out


def total_passes(wordlen, word, other, scores, threshold, use_dropoff):
    """Whether the WHOLE word's score passes (what a test on totals alone would accept): not the reference's rule."""
    t = sum(scores[c][c] for c in word) - threshold if use_dropoff else threshold
    return sum(scores[a][b] for a, b in zip(word, other)) >= t


def code_of(width, word):
    code = 0
    for c in word:
        code = code * width + c
    return code


def build(width, wordlen, strings, sources, scores=None, threshold=0, use_dropoff=True):
    """{"codes", "own", "sources", "emit_first", "emits", "n_links"}: the table's words by code ascending; own[k] the word's
    own seeds, sources[k] the codes of the words whose seed lists follow, in order; emits flattened."""
    own, first_g, words, order = {}, {}, {}, []
    g = 0
    for s, (pair, scale, offset) in zip(strings, sources):
        run = 0
        for i, c in enumerate(s):
            run = run + 1 if c else 0
            if run < wordlen:
                continue
            pos = i - wordlen + 1
            w = tuple(s[pos:i + 1])
            code = code_of(width, w)
            own.setdefault(code, []).insert(0, (pair, pos * scale + offset))
            if code not in first_g:
                first_g[code] = g
                words[code] = w
                order.append(code)
            g += 1
    nbrs, n_links = {}, 0
    if scores is not None:
        for code in order:                                                   # first(W) ascending; each list is prepended to
            for n in hood(width, wordlen, words[code], scores, threshold, use_dropoff):
                nc = code_of(width, n)
                if nc == code:
                    continue                                                 # seeder.c:470
                nbrs.setdefault(nc, []).insert(0, code)
                n_links += 1
    codes = sorted(set(own) | set(nbrs))
    emit_first, emits = [0], []
    for c in codes:
        emits += own.get(c, [])
        for w in nbrs.get(c, []):
            emits += own[w]
        emit_first.append(len(emits))
    return {"codes": codes, "own": [own.get(c, []) for c in codes], "sources": [nbrs.get(c, []) for c in codes],
            "emit_first": emit_first, "emits": emits, "n_links": n_links, "n_occurrences": g, "n_seeded_words": len(order)}


# ---- golden records ----------------------------------------------------------------------------------------------------------
def columns(match, automaton):
    """letter -> column.  The trie numbers the members by byte value DESCENDING (FSM_create, fsm.c:32-37); the compact
    automaton in member order (VFSM_create, vfsm.c:62-63)."""
    members = MEMBERS[match]
    if automaton == "fsm":
        return {ch: k + 1 for k, ch in enumerate(sorted(members, reverse=True))}
    return {ch: k + 1 for k, ch in enumerate(members)}


_SCORING = None


def column_scores(match, automaton):
    """s[a][b] over columns from the default matrices (tests/golden/scoring_data.json: nucleic / blosum62 through submat_index)."""
    global _SCORING
    if _SCORING is None:
        with open(os.path.join(GOLDEN, "scoring_data.json")) as f:
            _SCORING = json.load(f)
    mat = _SCORING["nucleic" if match == "dna2dna" else "blosum62"]
    idx = _SCORING["submat_index"]
    col = columns(match, automaton)
    width = len(col) + 1
    s = [[0] * width for _ in range(width)]
    for a, ca in col.items():
        for b, cb in col.items():
            s[ca][cb] = mat[idx[ord(a)]][idx[ord(b)]]
    return s


def record_flags(extra):
    """{"wordlen": n or None, "limit": n or None, "use_dropoff": bool} from a refdump flag list."""
    f = {"wordlen": None, "limit": None, "use_dropoff": True}
    extra = list(extra)
    for k, a in enumerate(extra):
        if a in ("--dnawordlen", "--proteinwordlen"):
            f["wordlen"] = int(extra[k + 1])
        elif a in ("--dnawordlimit", "--proteinwordlimit"):
            f["limit"] = int(extra[k + 1])
        elif a == "--useworddropoff":
            f["use_dropoff"] = extra[k + 1].lower() in ("yes", "true", "y", "t", "1")
    return f


def record_input(rec, flags):
    """A golden record's queries as the arguments of build() / Engine.wordtab_build: (width, wordlen, strings, sources, scores,
    threshold, use_dropoff).  The unmasked alphabets fold case (Sequence_mask: to upper); a residue outside the comparison
    alphabet is column 0 (seeder.c:501-514)."""
    f = record_flags(flags)
    match = rec["match"]
    col = columns(match, rec["automaton"])
    width, wordlen = len(col) + 1, rec["wordlen"]
    assert width == rec["width"] and (f["wordlen"] or DEFAULTS[match]["wordlen"]) == wordlen
    limit = DEFAULTS[match]["limit"] if f["limit"] is None else f["limit"]
    strings = [bytes(col.get(ch.upper(), 0) for ch in q) for q in rec["queries"]]
    sources = [(k, 1, 0) for k in range(len(strings))]
    scores = None if (f["use_dropoff"] and not limit) else column_scores(match, rec["automaton"])      # hspset.c:151
    return width, wordlen, strings, sources, scores, limit, f["use_dropoff"]


def record_table(rec):
    """What a record says the table is, in build()'s form (its words come code ascending off the trie / the leaf table)."""
    words = rec["words"]
    codes = [w[0] for w in words]
    assert codes == sorted(codes)
    own = [[tuple(s) for s in w[1]] for w in words]
    emit_first, emits = [0], []
    for w in words:
        emits += [tuple(s) for s in w[1]]
        for v in w[2]:
            emits += [tuple(s) for s in words[v][1]]
        emit_first.append(len(emits))
    keep = [k for k in range(len(words)) if emit_first[k + 1] > emit_first[k]]
    return {"codes": [codes[k] for k in keep], "own": [own[k] for k in keep],
            "sources": [[codes[v] for v in words[k][2]] for k in keep],
            "emit_first": [emit_first[k] for k in keep] + [len(emits)], "emits": emits}


# the flags the six seeds_* sets were made with (tools/make_golden.py:928-932)
SEEDS_FLAGS = {
    "seeds_dna2dna": (),
    "seeds_dna2dna_w9": ("--dnawordlen", "9"),
    "seeds_dna2dna_compact": ("--forcefsm", "compact"),
    "seeds_dna2dna_hood": ("--dnawordlen", "8", "--dnawordlimit", "5"),
    "seeds_protein2protein": ("--proteinwordlimit", "2"),
    "seeds_protein2protein_compact": ("--proteinwordlimit", "1", "--forcefsm", "compact"),
}


def load(name):
    with open(os.path.join(GOLDEN, name + ".jsonl")) as f:
        return [json.loads(l) for l in f if l.strip()]


def wordtab_sets():
    return sorted(f[:-6] for f in os.listdir(GOLDEN) if f.startswith("wordtab_") and f.endswith(".jsonl"))


def all_records():
    """(set name, flags, record) of every seeds_* and wordtab_* record (a wordtab record carries its own flags)."""
    out = []
    for name in sorted(SEEDS_FLAGS):
        out += [(name, SEEDS_FLAGS[name], r) for r in load(name)]
    for name in wordtab_sets():
        out += [(name, tuple(r["flags"]), r) for r in load(name)]
    return out
