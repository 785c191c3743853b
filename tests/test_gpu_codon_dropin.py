"""`exonerate-gpu --model coding2coding | ungapped:trans --exhaustive yes` (the reference's own binary with
integration/c4gpu_shim.c linked in): stdout byte-identical to the unmodified reference with its compiled CPU Viterbi
(oracle/_ref/exonerate-compiled), every pair and every strand combination served by the device; and one heuristic run, where
the seams decline a model whose query advance exceeds one and the output is the reference's.  Both binaries are built in the
build container and travel with the repo."""
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
_NCBI = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODONS = {}
for _i, _a in enumerate("TCAG"):
    for _j, _b in enumerate("TCAG"):
        for _k, _c in enumerate("TCAG"):
            CODONS.setdefault(_NCBI[_i * 16 + _j * 4 + _k], []).append(_a + _b + _c)


def _inputs(seed, n, reverse=False, lo=25, hi=60):
    """n homologous coding pairs: substitutions, a codon indel, a one- or two-base frameshift on one axis, off-frame flanks."""
    rng = random.Random(seed)
    rnd = lambda k: "".join(rng.choice("ACGT") for _ in range(k))
    qs, ts = [], []
    for k in range(n):
        pep = [rng.choice(AA) for _ in range(rng.randint(lo, hi))]
        qc = [rng.choice(CODONS[a]) for a in pep]
        tc = [rng.choice(CODONS[rng.choice(AA) if rng.random() < 0.08 else a]) for a in pep]
        at = rng.randint(5, len(pep) - 5)
        (qc if k % 2 else tc)[at:at] = [rng.choice(CODONS[rng.choice(AA)])]
        at = rng.randint(5, len(pep) - 5)
        (tc if k % 2 else qc)[at] += rnd(1 + k % 2)
        q = rnd(rng.randint(0, 4)) + "".join(qc) + rnd(rng.randint(0, 4))
        t = rnd(rng.randint(0, 20)) + "".join(tc) + rnd(rng.randint(0, 20))
        if reverse and k == 0:
            t = t.translate(COMP)[::-1]
        qs.append(("qy%d" % k, q))
        ts.append(("tg%d" % k, t))
    return qs, ts


def _write(tmp_path, qs, ts):
    qf, tf = str(tmp_path / "q.fa"), str(tmp_path / "t.fa")
    for path, recs in ((qf, qs), (tf, ts)):
        with open(path, "w") as f:
            for name, seq in recs:
                f.write(">%s\n%s\n" % (name, seq))
    return qf, tf


REPORTS = ["--showalignment", "yes", "--showvulgar", "yes", "--showcigar", "yes", "--showsugar", "yes", "--showtargetgff", "yes",
           "--showquerygff", "yes", "--ryo", "ryo: %s %pi %et %em %V\\n", "-V", "0"]


@needs_binaries
@pytest.mark.parametrize("model,extra,batch", [
    ("coding2coding", ["-S", "no"], "4096"),
    ("coding2coding", ["-S", "no", "--codongapopen", "-11", "--codongapextend", "-3", "--frameshift", "-13", "--proteinsubmat", "pam250"], "3"),
    ("coding2coding", ["-S", "no", "-D", "0"], "0"),                # C4GPU_BATCH=0: the per-call seam
    ("ungapped:trans", ["-S", "no", "--proteinsubmat", "pam250"], "4096"),
])
def test_exhaustive_runs_are_byte_identical_and_served_by_the_device(tmp_path, model, extra, batch):
    qs, ts = _inputs(77 + len(model) + len(extra), 3, reverse=True)
    qf, tf = _write(tmp_path, qs, ts)
    args = ["-m", model, "-E", "yes"] + REPORTS + extra + [qf, tf]
    ref = subprocess.Popen([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                         env=dict(os.environ, C4GPU_VERBOSE="1", C4GPU_BATCH=batch, C4GPU_MIN_CELLS="0"))
    ref_out, ref_err = ref.communicate(timeout=900)
    assert ref.returncode == 0, ref_err.decode()[-1500:]
    err = gpu.stderr.decode()
    assert gpu.returncode == 0, err[-2000:]
    assert gpu.stdout == ref_out
    out = ref_out.decode()
    vul = [l.split() for l in out.splitlines() if l.startswith("vulgar:")]
    assert len(vul) >= len(qs) and all(set(f[10::3]) <= {"C", "G", "F"} for f in vul)
    assert any("-" in (f[4], f[8]) for f in vul) and any((f[4], f[8]) == ("+", "+") for f in vul)
    if model == "coding2coding":
        assert re.search(r"vulgar: .* F \d+ \d+", out) and re.search(r"vulgar: .* G \d+ \d+", out)
    # every pair served by the device: no call and no batch fell back to the CPU Viterbi
    assert "c4gpu:" in err and "using the CPU" not in err and "falls back" not in err, err[-2000:]
    if batch != "0":
        # translate_both: the reference compares each pair on the four strand combinations (both sequences reversed)
        served = sum(int(m) for m in re.findall(r"c4gpu: batch of (\d+) pairs", err))
        assert served == len(qs) * len(ts) * 4, err[-2000:]
    else:
        name = "coding2coding" if model == "coding2coding" else "ungapped:codon"
        assert "c4gpu: batch of" not in err and len(re.findall(r"c4gpu: %s mode \d" % re.escape(name), err)) >= len(qs) * len(ts), err[-2000:]


@needs_binaries
@pytest.mark.parametrize("gapped", ["yes"])
def test_heuristic_runs_stay_on_the_reference(tmp_path, gapped):
    """The default (heuristic) mode: seeding, HSP extension, BSDP and SDP decline a model whose max_query_advance is 3, so the
    run is the reference's own code from end to end -- same bytes, nothing served by a seam."""
    qs, ts = _inputs(5, 3, lo=60, hi=90)
    qf, tf = _write(tmp_path, qs, ts)
    args = ["-m", "coding2coding", "--gappedextension", gapped] + REPORTS + [qf, tf]
    ref = subprocess.run([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                         env=dict(os.environ, C4GPU_VERBOSE="1", C4GPU_BATCH="4096"))
    assert ref.returncode == 0 and gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    assert gpu.stdout == ref.stdout and b"vulgar:" in ref.stdout
    err = gpu.stderr.decode()
    # the seams print a summary only for what they served (integration/c4gpu_{hsp,seed,sdp,bsdp}.c): none may appear, and no
    # Viterbi call may have been tried on the device and handed back
    for seam in ("c4gpu hsp:", "c4gpu sdp:", "c4gpu bsdp:", "targets walked in", "c4gpu: batch of", "using the CPU Viterbi"):
        assert seam not in err, err[-1500:]
