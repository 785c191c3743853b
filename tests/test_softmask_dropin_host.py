"""Soft-masked runs through the drop-in binary, checked WITHOUT a device: --softmasktarget / --softmaskquery with the
seams in their host modes (C4GPU_HSP_HOST=1: the two-stage extension of hspset.c:981-995 comes from the reference's own
HSPset_seed_hsp on scratch sets run with the real threshold; the replay stores nothing for a dropped seed and moves its
horizon to the masked end).  Byte for byte against the unmodified reference.  It is also the first run of the word-scan, SDP
and BSDP seams on lower-case input (C4GPU_SEED_CHECK=1 compares every seed with the reference's own walk).  The device
route: test_gpu_softmask_dropin.py."""
import os, random, re, subprocess
import pytest

from test_integration_bsdp_host import heuristic_inputs, GPU_EXE, CPU_EXE

pytestmark = pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                reason="reference binaries are built in the build container (make -C integration)")

HOST_ENV = {"C4GPU_HSP_HOST": "1", "C4GPU_SDP_HOST": "1", "C4GPU_BSDP_HOST": "1", "C4GPU_SEED_HOST": "1", "C4GPU_SEED_FACTOR": "0",
            "C4GPU_SEED_CHECK": "1", "C4GPU_HSP_CHECK": "1"}
MASKS = {"target": ["--softmasktarget", "yes"], "query": ["--softmaskquery", "yes"],
         "both": ["--softmaskquery", "yes", "--softmasktarget", "yes"]}


def soften(rng, seq, mean_upper, mean_lower):
    """Runs of lower case (soft-masked repeats) between upper-case islands of every length from 1 up."""
    out, low, left = [], False, rng.randint(1, mean_upper)
    for c in seq:
        if left == 0:
            low = not low
            left = rng.randint(1, 2 * (mean_lower if low else mean_upper))
        out.append(c.lower() if low else c)
        left -= 1
    return "".join(out)


def softmask_inputs(model, n, seed):
    """The related pairs of the other seam tests with lower-case runs over BOTH sides (a side without its option is not
    masked, whatever its case), the wildcard in lower case here and there (never masked, alphabet.c:124-129)."""
    qs, ts = heuristic_inputs(model, n, seed)
    rng = random.Random(seed + 1)
    protein = model.startswith("protein")
    qs = [(name, soften(rng, q, 12 if protein else 40, 6 if protein else 25)) for name, q in qs]
    ts = [(name, soften(rng, t.replace("ACG", "ACn", 2), 24 if protein else 40, 5 if protein else 25)) for name, t in ts]
    return qs, ts


def run_softmask(tmp_path, exes_env, model, gapped, mask, n=4, seed=5, extra=()):
    qs, ts = softmask_inputs(model, n, seed)
    qf, tf = str(tmp_path / "q.fa"), str(tmp_path / "t.fa")
    for path, recs in ((qf, qs), (tf, ts)):
        with open(path, "w") as f:
            for name, seq in recs:
                f.write(">%s\n%s\n" % (name, seq))
    # (most six-residue protein words reach the default threshold of 30 by themselves: 45 there, so that islands end under it)
    extra = list(extra) + (["--proteinhspthreshold", "45"] if model.startswith("protein") else [])
    args = ["-m", model, "--gappedextension", gapped, "--showalignment", "yes", "--showvulgar", "yes", "-V", "0"] + MASKS[mask] + \
           extra + [qf, tf]
    ref = subprocess.run([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                         env=dict(os.environ, C4GPU_VERBOSE="1", **exes_env))
    assert ref.returncode == 0, ref.stderr.decode()[-800:]
    assert gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    return ref.stdout, gpu.stdout, gpu.stderr.decode()


def hsp_line(err):
    m = re.search(r"c4gpu hsp: (\d+) word hits of (\d+) HSP sets extended in (\d+) device batch.*?(\d+) HSPs passed their horizon, "
                  r"(\d+) seeds dropped at masked ends, (\d+) checked against the reference", err)
    assert m, err[-1500:]
    return dict(zip(("hits", "sets", "batches", "stored", "dropped", "checked"), (int(x) for x in m.groups())))


@pytest.mark.parametrize("gapped", ["no", "yes"])
@pytest.mark.parametrize("mask", ["target", "query", "both"])
@pytest.mark.parametrize("model", ["est2genome", "affine:local", "protein2genome", "protein2dna"])
def test_softmasked_runs_are_byte_identical_with_host_extensions(tmp_path, model, mask, gapped):
    ref, gpu, err = run_softmask(tmp_path, HOST_ENV, model, gapped, mask)
    assert gpu == ref and ref.count(b"vulgar:") >= 2
    line = hsp_line(err)
    assert line["hits"] > 50 and line["stored"] > 0
    if mask != "query":                       # (an unmasked target lets most seeds of a masked query grow past the threshold)
        assert line["dropped"] > 0, err[-600:]
    assert "every seed equal to the reference's own walk" in err


def test_a_run_without_the_option_drops_nothing(tmp_path):
    """Lower case without --softmask*: not masked (Alphabet_is_masked); the old extension path, no dropped seed."""
    qs, ts = softmask_inputs("est2genome", 4, 5)
    qf, tf = str(tmp_path / "q.fa"), str(tmp_path / "t.fa")
    for path, recs in ((qf, qs), (tf, ts)):
        with open(path, "w") as f:
            for name, seq in recs:
                f.write(">%s\n%s\n" % (name, seq))
    args = ["-m", "est2genome", "--showalignment", "yes", "--showvulgar", "yes", "-V", "0", qf, tf]
    ref = subprocess.run([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                         env=dict(os.environ, C4GPU_VERBOSE="1", **HOST_ENV))
    assert ref.returncode == 0 and gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    assert gpu.stdout == ref.stdout and ref.stdout.count(b"vulgar:") >= 2
    assert hsp_line(gpu.stderr.decode())["dropped"] == 0
