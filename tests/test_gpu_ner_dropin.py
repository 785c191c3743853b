"""`exonerate-gpu --model ner --exhaustive yes` (the reference's own binary with integration/c4gpu_shim.c linked in): stdout
byte-identical to the unmodified reference with its compiled CPU Viterbi (oracle/_ref/exonerate-compiled), every pair served by
the device.  Both binaries are built in the build container and travel with the repo."""
import os, random, re, subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_EXE = os.path.join(ROOT, "integration", "_build", "exonerate-gpu")
CPU_EXE = os.path.join(ROOT, "oracle", "_ref", "exonerate-compiled")
needs_binaries = pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                    reason="reference binaries are built in the build container (make -C integration)")
COMP = str.maketrans("ACGT", "TGCA")
AA = "ARNDCQEGHILKMFPSTWYV"


def _inputs(kind, seed, n=3, blocks=(60, 140)):
    rng = random.Random(seed)
    alpha = AA if kind == "protein" else "ACGT"
    rnd = lambda k: "".join(rng.choice(alpha) for _ in range(k))
    mut = lambda s, r: "".join((rng.choice(alpha) if rng.random() < r else c) for c in s)
    qs, ts = [], []
    for k in range(n):
        b = [rnd(rng.randint(*blocks)) for _ in range(3)]
        q = rnd(rng.randint(5, 30)) + b[0] + rnd(rng.randint(8, 40)) + b[1] + rnd(rng.randint(8, 40)) + b[2] + rnd(rng.randint(5, 30))
        t = rnd(rng.randint(30, 200)) + mut(b[0], 0.05) + rnd(rng.randint(41, 70)) + mut(b[1], 0.05) + rnd(rng.randint(3, 7)) + \
            mut(b[2], 0.05) + rnd(rng.randint(30, 200))
        if kind == "reverse":
            t = t.translate(COMP)[::-1]               # the best hit is then on the reverse strand
        elif kind == "repeat" and k == 1:
            t += rnd(40) + mut(b[0] + rnd(12) + b[1], 0.08)      # a second copy: later rounds of the sub-optimal loop
        qs.append(("qy%d" % k, q))
        ts.append(("tg%d" % k, t))
    return qs, ts


@needs_binaries
@pytest.mark.parametrize("kind,extra,batch", [
    ("repeat", [], "4096"),                                        # defaults: --subopt yes
    ("repeat", ["--neropen", "-35", "-n", "2"], "4096"),
    ("protein", [], "4096"),
    ("reverse", ["-S", "no"], "4096"),
    ("repeat", ["-S", "no"], "0"),                                 # C4GPU_BATCH=0: the per-call seam
])
def test_exhaustive_ner_is_byte_identical_and_served_by_the_device(tmp_path, kind, extra, batch):
    # (the reference's sub-optimal loop is the slow side of this test: two shorter sequences a side there)
    subopt_all = "-S" not in extra and "-n" not in extra
    qs, ts = _inputs(kind, 31 + len(kind), 2 if subopt_all else 3, (40, 70) if subopt_all else (60, 140))
    qf, tf = str(tmp_path / "q.fa"), str(tmp_path / "t.fa")
    for path, recs in ((qf, qs), (tf, ts)):
        with open(path, "w") as f:
            for name, seq in recs:
                f.write(">%s\n%s\n" % (name, seq))
    args = ["-m", "ner", "-E", "yes", "--showalignment", "yes", "--showvulgar", "yes", "--showcigar", "yes", "--showsugar", "yes",
            "--showtargetgff", "yes", "--showquerygff", "yes", "--ryo", "ryo: %s %pi %et %em %V\\n", "-V", "0"] + extra + [qf, tf]
    ref = subprocess.Popen([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                         env=dict(os.environ, C4GPU_VERBOSE="1", C4GPU_BATCH=batch))
    ref_out, ref_err = ref.communicate(timeout=900)
    assert ref.returncode == 0, ref_err.decode()[-1500:]
    err = gpu.stderr.decode()
    assert gpu.returncode == 0, err[-2000:]
    assert gpu.stdout == ref_out
    out = ref_out.decode()
    assert out.count("vulgar:") >= len(qs) and re.search(r"vulgar: .* N \d+ \d+", out)
    if kind == "reverse":              # (for two DNA sequences the reference turns the query round: the hit is on its '-' strand)
        best = max((l.split() for l in out.splitlines() if l.startswith("vulgar:")), key=lambda f: int(f[9]))
        assert "-" in (best[4], best[8]), best[:10]
    # every pair served by the device: no call and no batch fell back to the CPU Viterbi
    assert "c4gpu:" in err and "using the CPU" not in err and "falls back" not in err, err[-2000:]
    if batch != "0":
        served = sum(int(m) for m in re.findall(r"c4gpu: batch of (\d+) pairs", err))
        strands = 1 if kind == "protein" else 2
        assert served == len(qs) * len(ts) * strands, err[-2000:]
    else:
        assert "c4gpu: batch of" not in err and len(re.findall(r"c4gpu: NER:affine:local:\S+ mode \d", err)) >= len(qs) * len(ts), err[-2000:]
