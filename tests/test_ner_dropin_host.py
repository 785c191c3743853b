"""Heuristic `--model ner` runs of the drop-in binary stay on the reference's own functions.  The ner state is a span on BOTH
axes (ner.c:105); the device SDP passes have no spans along the query and BSDP has no compiled families for such a span, so
the two heuristic seams (integration/c4gpu_sdp.c, c4gpu_bsdp.c) decline the model by that property
(shim_model_has_query_span) although it flattens since the exhaustive route serves it.  Checked WITHOUT a device, with the
seams' host modes (C4GPU_BSDP_HOST=1 / C4GPU_SDP_HOST=1: the seam's bookkeeping around the reference's own DPs): output
byte-identical to the unmodified reference, and the seams' counters show that they took nothing."""
import os, random, re, subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_EXE = os.path.join(ROOT, "integration", "_build", "exonerate-gpu")
CPU_EXE = os.path.join(ROOT, "oracle", "_ref", "exonerate-compiled")
pytestmark = pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                reason="reference binaries are built in the build container (make -C integration)")


def _inputs(n, seed):
    """Conserved blocks long enough to seed HSPs, with unrelated inserts of different lengths between them."""
    rng = random.Random(seed)
    dna = lambda k: "".join(rng.choice("ACGT") for _ in range(k))
    mut = lambda s, r: "".join((rng.choice("ACGT") if rng.random() < r else c) for c in s)
    qs, ts = [], []
    for k in range(n):
        b = [dna(rng.randint(120, 260)) for _ in range(3)]
        q = dna(rng.randint(20, 80)) + b[0] + dna(rng.randint(15, 45)) + b[1] + dna(rng.randint(15, 45)) + b[2] + dna(rng.randint(20, 80))
        t = dna(rng.randint(100, 900)) + mut(b[0], 0.04) + dna(rng.randint(50, 90)) + mut(b[1], 0.04) + dna(rng.randint(12, 14)) + \
            mut(b[2], 0.04) + dna(rng.randint(100, 900))
        qs.append(("q%d" % k, q))
        ts.append(("t%d" % k, t))
    return qs, ts


def _run_both(tmp_path, extra, env_extra):
    qs, ts = _inputs(5, 23)
    qf, tf = str(tmp_path / "q.fa"), str(tmp_path / "t.fa")
    for path, recs in ((qf, qs), (tf, ts)):
        with open(path, "w") as f:
            for name, seq in recs:
                f.write(">%s\n%s\n" % (name, seq))
    args = ["-m", "ner", "--showalignment", "yes", "--showvulgar", "yes", "-V", "0"] + list(extra) + [qf, tf]
    ref = subprocess.run([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                         env=dict(os.environ, C4GPU_VERBOSE="1", **env_extra))
    assert ref.returncode == 0, ref.stderr.decode()[-800:]
    assert gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    return ref.stdout, gpu.stdout, gpu.stderr.decode()


@pytest.mark.parametrize("extra", [[], ["-S", "no"], ["--neropen", "-35", "--bestn", "1"]])
def test_bsdp_seam_declines_ner(tmp_path, extra):
    ref, gpu, err = _run_both(tmp_path, ["--gappedextension", "no"] + extra, {"C4GPU_BSDP_HOST": "1"})
    assert gpu == ref
    assert ref.count(b"vulgar:") >= 3
    # shim_bsdp_report prints its line only for runs in which the seam collected a pair
    assert "c4gpu bsdp:" not in err, err[-1500:]
    assert not re.search(r"[1-9]\d* candidate sub-DPs", err), err[-1500:]


@pytest.mark.parametrize("extra", [[], ["-S", "no"], ["--neropen", "-35", "--bestn", "1"]])
def test_sdp_seam_declines_ner(tmp_path, extra):
    ref, gpu, err = _run_both(tmp_path, ["--gappedextension", "yes"] + extra, {"C4GPU_SDP_HOST": "1"})
    assert gpu == ref
    assert ref.count(b"vulgar:") >= 3
    # shim_sdp_report prints its line only for runs in which the seam took a pair
    assert "c4gpu sdp:" not in err, err[-1500:]
    assert not re.search(r"c4gpu sdp: [1-9]\d* pairs", err), err[-1500:]


def test_the_seams_do_take_the_model_next_door(tmp_path):
    """The same inputs under affine:local ARE collected by both seams: the two assertions above cannot pass because the
    reports went missing."""
    qs, ts = _inputs(5, 23)
    qf, tf = str(tmp_path / "q.fa"), str(tmp_path / "t.fa")
    for path, recs in ((qf, qs), (tf, ts)):
        with open(path, "w") as f:
            for name, seq in recs:
                f.write(">%s\n%s\n" % (name, seq))
    for mode, var, tag in (("no", "C4GPU_BSDP_HOST", "c4gpu bsdp: "), ("yes", "C4GPU_SDP_HOST", "c4gpu sdp: ")):
        args = ["-m", "affine:local", "--gappedextension", mode, "--showvulgar", "yes", "-V", "0", qf, tf]
        gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                             env=dict(os.environ, C4GPU_VERBOSE="1", **{var: "1"}))
        assert gpu.returncode == 0, gpu.stderr.decode()[-1500:]
        m = re.search(re.escape(tag) + r"(\d+) pairs", gpu.stderr.decode())
        assert m and int(m.group(1)) >= 3, gpu.stderr.decode()[-1500:]
