"""Inputs and the runner of the drop-in tests of the fused seeding route under --softmaskquery / --softmasktarget / --seedrepeat
(tests/test_integration_seed_fused_opt_host.py, _gpu.py).  No tests here.

Small DNA and protein inputs on which every one of the options decides what the reference prints: a copy that is lower case but
for an island too short to reach the HSP threshold (lost with the side's softmask option), the same on the query side, a copy of
exactly one word (lost at --seedrepeat 2), and plain copies that every run keeps."""
import os
import random
import re
import subprocess

from test_integration_bsdp_host import GPU_EXE, CPU_EXE

AA = "ARNDCQEGHILKMFPSTWYV"
KINDS = {"dna": dict(alphabet="ACGT", w=12, qlen=150, island=None, strong=None, flags=["-Q", "dna", "-T", "dna"]),
         "protein": dict(alphabet=AA, w=6, qlen=70, island="AILVSA", strong="WCHFYMWCHFYM",
                         flags=["-Q", "protein", "-T", "protein", "--proteinwordlimit", "0"])}
OPTIONS = [["--softmasktarget", "yes"], ["--softmaskquery", "yes"], ["--softmaskquery", "yes", "--softmasktarget", "yes"],
           ["--seedrepeat", "2"], ["--seedrepeat", "2", "--softmasktarget", "yes"]]


def inputs(kind):
    """(queries, targets) as [(name, sequence)], for the default HSP thresholds (75 for DNA, 30 for protein).
    Query 0: its copy in target 0 is lower case around an island of one word and a symbol (DNA: 13 * 5 = 65; protein: six weak
    residues, 24) -- lost with --softmasktarget.  Query 1: itself lower case around such an island -- lost with --softmaskquery.
    Query 2: target 1 holds one word of it, a mismatch, and a few more symbols: one word hit, an HSP over the threshold -- lost
    at --seedrepeat 2.  Query 3: plain copies in both targets, a lower-case stretch inside one of them."""
    k = KINDS[kind]
    rng = random.Random(8100 + len(kind))
    a, w, n = k["alphabet"], k["w"], k["qlen"]
    rand = lambda m: "".join(rng.choice(a) for _ in range(m))
    other = lambda c: rng.choice([x for x in a if x != c])
    q = [rand(n) for _ in range(4)]
    isl = w + 1 if kind == "dna" else w
    if k["island"]:
        q[0] = q[0][:50] + k["island"] + q[0][50 + isl:]
        q[1] = q[1][:30] + k["island"] + q[1][30 + isl:]
        q[2] = q[2][:40] + k["strong"] + q[2][40 + len(k["strong"]):]
    around = lambda s, at: s[:at].lower() + s[at:at + isl] + s[at + isl:].lower()
    q[1] = around(q[1], 30)
    tail = w - 1 if kind == "protein" else 8
    once = q[2][40:40 + w] + other(q[2][40 + w]) + q[2][41 + w:41 + w + tail]
    t0 = rand(37) + around(q[0], 50) + rand(23) + q[1].upper() + rand(31) + q[3] + rand(12)
    copy3 = q[3][:60] + q[3][60:80].lower() + q[3][80:]
    t1 = rand(29) + other(q[2][39]) + once + other(q[2][41 + w + tail]) + rand(45) + copy3 + rand(17)
    return [("q%d" % i, s) for i, s in enumerate(q)], [("t0", t0), ("t1", t1)]


def run(tmp_path, kind, option, env_extra):
    """stdout of the reference binary and of the drop-in (and the drop-in's stderr) for -m ungapped with `option`; option None:
    the reference alone, without any of the options."""
    qs, ts = inputs(kind)
    qf, tf = str(tmp_path / ("q_%s.fa" % kind)), str(tmp_path / ("t_%s.fa" % kind))
    for path, recs in ((qf, qs), (tf, ts)):
        with open(path, "w") as f:
            for name, seq in recs:
                f.write(">%s\n%s\n" % (name, seq))
    args = ["-m", "ungapped"] + KINDS[kind]["flags"] + ["--showalignment", "no", "--showsugar", "yes", "--showvulgar", "no", "--score", "1",
                                                       "-V", "0"]
    args += list(option or []) + [qf, tf]
    ref = subprocess.run([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert ref.returncode == 0, ref.stderr.decode()[-800:]
    if option is None:
        return ref.stdout
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                         env=dict(os.environ, C4GPU_VERBOSE="1", **env_extra))
    assert gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    return ref.stdout, gpu.stdout, gpu.stderr.decode()


def fused_line(err):
    m = re.search(r"c4gpu seed fused: (\d+) targets through c4gpu_seed_extend: (\d+) word hits, (\d+) extensions, (\d+) HSPs kept", err)
    assert m, err[-1500:]
    return [int(x) for x in m.groups()]
