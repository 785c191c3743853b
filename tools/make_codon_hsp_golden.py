#!/usr/bin/env python3
"""Fixtures of the codon HSP seam (Match_Type_CODON2CODON: the seeds of ungapped:trans and coding2coding).

Runs the drop-in binary with C4GPU_CODON_SEED=1 C4GPU_HSP_HOST=1 C4GPU_SEED_OFF=1 C4GPU_HSP_DUMP=FILE: the word hits are the
reference's own walk, every extension is the reference's own HSPset_seed_hsp on a scratch set, so every number in the dump comes
from the reference's functions; the run's stdout must equal the unmodified reference's (oracle/_ref/exonerate).  Writes
    tests/golden/hsp_codon.jsonl            the sets of the runs without soft-masking, in the shape of the other hsp_*.jsonl
    tests/golden/hsp_codon_softmask.jsonl   the sets of the soft-masked runs (each record carries its two mask flags)
    tests/golden/codon_hsp_cli.json         the inputs and the sugar lines of the pure reference binary for the same runs
Needs the reference binaries (built where the reference tree is: __graft_entry__.build())."""
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_EXE = os.path.join(ROOT, "integration", "_build", "exonerate-gpu")
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "exonerate")
GOLDEN = os.path.join(ROOT, "tests", "golden")
TABLE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
SENSE = [a + b + c for a in "TCAG" for b in "TCAG" for c in "TCAG" if TABLE["TCAG".index(a) * 16 + "TCAG".index(b) * 4 + "TCAG".index(c)] != "*"]


def orf(rng, n):
    return "".join(rng.choice(SENSE) for _ in range(n))


def other(rng, c):
    return rng.choice([x for x in "ACGT" if x != c])


def lower_except(s, keep):
    return "".join(c if any(a <= i < b for a, b in keep) else c.lower() for i, c in enumerate(s))


def cases(seed):
    """name -> (query, target, extra arguments, masked)."""
    rng = random.Random(seed)
    q = orf(rng, 100)
    tail = list(q[-120:])
    for at in rng.sample(range(10, 110), 3):
        tail[at] = other(rng, tail[at])
    a_t = "G" + "".join(tail) + "TT"
    islands = [(30, 48), (90, 114), (180, 300)]
    b_t = lower_except(q, islands)
    # (the query stays upper case: with lower case under --softmaskquery the reference itself stops in HSP_init -- "Initial
    # HSP score [-1] less than zero" -- on the seeds its masked word lists make; the flag still sends the set down the masked path)
    b_q = q
    c_t = "AC" + "".join(other(rng, c) if i % 17 == 16 else c for i, c in enumerate(q))
    q70 = orf(rng, 70)
    d_t = "A" + q70[30:150] + "G" + q70[:90]
    # E: 93 codons whose last 31 repeat the 31 before them, against the query's last 90 nt: every target position matches on
    # the diagonals -96 and -189.  Both sums are negative (3 * 96 > 279), the diagonals are qlen / 3 apart and in the same frames,
    # so the wrapped seeds of one land on the entry of the other and the second diagonal's seeds fall under the first one's horizon
    unit = orf(rng, 31)
    e_q = orf(rng, 31) + unit + unit
    e_t = e_q[189:279] + "TAAC"
    return {
        "E": (e_q, e_t, ["--score", "30"], False),
        "A": (q, a_t, ["--score", "30"], False),
        "B_t": (q, b_t, ["--softmasktarget", "yes", "--score", "30"], True),
        "B_qt": (b_q, b_t, ["--softmaskquery", "yes", "--softmasktarget", "yes", "--score", "30"], True),
        "C": (q, c_t, ["--score", "30"], False),
        "D": (q70, d_t, ["--score", "30"], False),
    }


def run_case(tmp, name, query, target, extra):
    qf, tf, dump = os.path.join(tmp, name + "_q.fa"), os.path.join(tmp, name + "_t.fa"), os.path.join(tmp, name + ".dump")
    with open(qf, "w") as f:
        f.write(">qy\n%s\n" % query)
    with open(tf, "w") as f:
        f.write(">tg\n%s\n" % target)
    args = ["-m", "ungapped:trans", "--showalignment", "no", "--showvulgar", "no", "--showsugar", "yes", "-V", "0"] + extra + [qf, tf]
    ref = subprocess.run([REF_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert ref.returncode == 0, ref.stderr.decode()[-800:]
    env = dict(os.environ, C4GPU_CODON_SEED="1", C4GPU_HSP_HOST="1", C4GPU_SEED_OFF="1", C4GPU_HSP_DUMP=dump, C4GPU_VERBOSE="1")
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    assert gpu.stdout == ref.stdout, (name, gpu.stdout, ref.stdout)
    assert "c4gpu hsp:" in gpu.stderr.decode(), gpu.stderr.decode()[-800:]
    with open(dump) as f:
        sets = [json.loads(l) for l in f if l.strip()]
    sugar = [l for l in ref.stdout.decode().splitlines() if l.startswith("sugar:")]
    return sets, sugar, args[:-2]


PARAM_KEYS = ["match", "seedlen", "dropoff", "threshold", "query_advance", "target_advance", "seed_repeat"]


def record(name, k, s):
    masked = s["mask_query"] or s["mask_target"]
    single, dropped_end = [], []
    for h in s["single"]:
        if h[5]:
            single.append(None)
            dropped_end.append(h[1])
        else:
            single.append(h[:5] if (masked or h[3] >= s["threshold"]) else None)
            dropped_end.append(None)
    # the set is dumped before it is finalised, its HSPs' cobs still 0 (HSPset_add_known_hsp leaves them to HSPset_finalise):
    # each takes the cobs of the per-seed record of the same HSP -- the seed the replay stored it for
    cobs = {tuple(h[:4]): h[4] for h in s["single"] if not h[5]}
    held = [h[:4] + [cobs[tuple(h[:4])]] for h in s["set"]]
    return {"id": "%s_%d" % (name, k), "mask_query": s["mask_query"], "mask_target": s["mask_target"], "single": single,
            "dropped_end": dropped_end, "set": held, "query": s["query"], "target": s["target"], "seeds": s["seeds"]}


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 20261020
    plain, soft, cli, params = [], [], {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (q, t, extra, masked) in cases(seed).items():
            assert len(q) <= 300
            sets, sugar, args = run_case(tmp, name, q, t, extra)
            cli[name] = {"query": q, "target": t, "args": args, "sugar": sugar}
            for k, s in enumerate(sets):
                assert s["match"] == "codon2codon" and s["seed_repeat"] == 1
                par = {key: s[key] for key in PARAM_KEYS}
                kind = "soft" if masked else "plain"
                assert params.setdefault(kind, par) == par, (name, par)
                (soft if masked else plain).append(record(name, k, s))
            print("%-5s %d sets, %d seeds, %d sugar lines: %s" % (name, len(sets), sum(len(s["seeds"]) for s in sets), len(sugar),
                                                                   sugar[:1]))
    for fname, kind, recs in (("hsp_codon.jsonl", "plain", plain), ("hsp_codon_softmask.jsonl", "soft", soft)):
        path = os.path.join(GOLDEN, fname)
        with open(path, "w") as f:
            f.write(json.dumps({"params": params[kind]}, separators=(",", ":")) + "\n")
            for r in recs:
                f.write(json.dumps(r, separators=(",", ":")) + "\n")
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 200 * 1024
    with open(os.path.join(GOLDEN, "codon_hsp_cli.json"), "w") as f:
        json.dump({"seed": seed, "runs": cli}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
