#!/usr/bin/env python3
"""Generate tests/golden/wordtab_*.jsonl: word tables with neighbourhoods read off the REFERENCE's own automaton
(`oracle/_ref/refdump --cmd seeds`: the words its queries put into the trie / the compact automaton's leaf table, each with its
own seeds and its neighbour words in list order, the target as automaton columns, and every HSPset_seed_hsp call its walk made).
Runs only where the reference binaries are built.  The records are the existing dump's, plus "flags" (what refdump was given),
"queries" and "target".

Sets (queries of at most 60 residues; every set holds two queries that share words, a query with a reset -- N / X --, and a
query shorter than a word, and three words one substitution away from a word of the first query):
    wordtab_protein             the default --proteinwordlimit (4)
    wordtab_protein_wide        --proteinwordlimit 6: table words with several neighbour sources
    wordtab_protein_abs         --useworddropoff no --proteinwordlimit 31: the limit as an absolute score
    wordtab_protein_compact     --proteinwordlimit 3 --forcefsm compact
    wordtab_dna_hood            --dnawordlen 6 --dnawordlimit 9: one mismatch costs 5 + 4 = 9 in the default matrix
    wordtab_dna_hood_compact    the same with --forcefsm compact
The script asserts what each set is there for (tests/wordtab_model.py decides) and refuses to write otherwise."""
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wordtab_model as wm                                           # noqa: E402

REFDUMP = os.path.join(ROOT, "oracle", "_ref", "refdump")
OUT = os.path.join(ROOT, "tests", "golden")
AA = "ARNDCQEGHILKMFPSTWYV"
SETS = (("wordtab_protein", "protein2protein", 1, 16, ()),
        ("wordtab_protein_wide", "protein2protein", 1, 12, ("--proteinwordlimit", "6")),
        ("wordtab_protein_abs", "protein2protein", 1, 16, ("--useworddropoff", "no", "--proteinwordlimit", "31")),
        ("wordtab_protein_compact", "protein2protein", 1, 16, ("--proteinwordlimit", "3", "--forcefsm", "compact")),
        ("wordtab_dna_hood", "dna2dna", 1, 28, ("--dnawordlen", "6", "--dnawordlimit", "9")),
        ("wordtab_dna_hood_compact", "dna2dna", 1, 28, ("--dnawordlen", "6", "--dnawordlimit", "9", "--forcefsm", "compact")))


def rand_seq(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, rate, alphabet):
    return "".join(rng.choice(alphabet) if rng.random() < rate else c for c in s)


def cases(kind, n, qlen, seed):
    rng = random.Random(seed)
    alphabet, reset, w = ("ACGT", "N", 6) if kind == "dna2dna" else (AA, "X", 6)
    out = []
    for k in range(n):
        q0 = rand_seq(rng, qlen, alphabet)
        cut = qlen // 2
        q1 = rand_seq(rng, 4, alphabet) + q0[cut - 5:cut + 6] + rand_seq(rng, 5, alphabet)       # shares words with q0
        q2 = q0[:w + 2] + reset + mutate(rng, q0[w + 3:qlen - 3], 0.15, alphabet)                # a reset; near copies of q0's words
        q3 = rand_seq(rng, w - 1, alphabet)                                                      # shorter than a word
        # three words one substitution (the best-scoring one) away from a word of q0: that word gets several neighbour sources
        col, sc = wm.columns(kind, "fsm"), wm.column_scores(kind, "fsm")
        word = q0[2:2 + w]
        near = []
        for p in (1, 3, 4):
            best = max((b for b in alphabet if b != word[p]), key=lambda b: (sc[col[word[p]]][col[b]], b))
            near.append(word[:p] + best + word[p + 1:])
        q4 = reset.join(near)
        t = rand_seq(rng, rng.randint(0, 9), alphabet) + mutate(rng, q0, 0.12, alphabet) + reset + q1[2:] + rand_seq(rng, 5, alphabet)
        qs = [q0, q1, q2, q3, q4]
        assert all(len(q) <= 60 for q in qs)
        out.append(("wt_%s%03d" % (kind[:3], k), qs, t))
    return out


def run(kind, cs, flags):
    with tempfile.NamedTemporaryFile("w", suffix=".tsv", delete=False) as f:
        for cid, qs, t in cs:
            f.write("%s\t%s\t%s\n" % (cid, ",".join(qs), t))
        path = f.name
    out = subprocess.run([REFDUMP, "--cmd", "seeds", "--model", kind, "--input", path] + list(flags),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout.decode()
    os.unlink(path)
    recs = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    assert len(recs) == len(cs)
    for r, (cid, qs, t) in zip(recs, cs):
        assert r["id"] == cid
        r["queries"], r["target"], r["flags"] = qs, t, list(flags)
    return recs


def main():
    for name, kind, n, qlen, flags in SETS:
        recs = run(kind, cases(kind, n, qlen, 1000 + len(name)), flags)
        links = sum(len(w[2]) for r in recs for w in r["words"])
        many = max(len(w[2]) for r in recs for w in r["words"])
        shared = any(len({q for q, _ in w[1]}) > 1 for r in recs for w in r["words"])
        assert links > 0 and shared, (name, links, shared)
        assert any(0 in r["symbols"] for r in recs) and all(len(r["expected"]) > 0 for r in recs), name
        if name == "wordtab_protein_wide":
            assert many >= 3, many
        for r in recs:                                               # the restatement must already agree
            got, exp = wm.build(*wm.record_input(r, flags)), wm.record_table(r)
            assert all(got[k] == exp[k] for k in ("codes", "own", "sources", "emit_first", "emits")), (name, r["id"])
        path = os.path.join(OUT, name + ".jsonl")
        with open(path, "w") as f:
            for r in recs:
                f.write(json.dumps(r, separators=(",", ":")) + "\n")
        size = os.path.getsize(path)
        assert size < 40 * 1024, (name, size)
        print(name, len(recs), "seeders,", sum(len(r["words"]) for r in recs), "words,", links, "neighbour links, at most", many,
              "sources a word,", sum(len(r["expected"]) for r in recs), "seeds,", size, "bytes", recs[0]["automaton"])


if __name__ == "__main__":
    main()
