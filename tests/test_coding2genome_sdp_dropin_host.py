"""The opt-in SDP seam of the drop-in binary for coding2genome (C4GPU_CODING2GENOME_SDP=1: a heuristic run with
--gappedextension yes, the default), checked WITHOUT a device: with C4GPU_SDP_HOST=1 the alignments behind the seam are the
reference's own SDP_Pair_next_path, so the seam's own work -- letting this wide model through, gathering the comparison's HSPs,
batching, the replay in submission order -- is exercised byte for byte against the unmodified reference.  Without the switch,
or with coding2coding's switch alone, nothing moves.  The device route: test_gpu_coding2genome_sdp_dropin.py."""
import os
import random
import subprocess

import pytest

import coding2genome_cases as cg
from test_codon_sdp_dropin_host import HOST, sdp_line
from test_gpu_codon_dropin import _write, GPU_EXE, CPU_EXE, REPORTS

pytestmark = pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                reason="reference binaries are built in the build container (make -C integration)")

SWITCH = dict(HOST, C4GPU_CODING2GENOME_SDP="1")


def inputs():
    """Three CDS and their gene-bearing targets: introns of all three phases, a frameshift and a codon gap among them; the first
    target reverse-complemented."""
    rng = random.Random(6161)
    shapes = [dict(n_aa=48, introns=[(16, 1, 70), (33, 0, 55)], events=[("t1", 25)]),
              dict(n_aa=56, introns=[(20, 2, 64)], events=[("qc", 40)], flank_q=1),
              dict(n_aa=40, introns=[(19, 0, 48)], flank_q=2)]
    qs, ts = [], []
    for k, sp in enumerate(shapes):
        q, t = cg.gene_pair(rng, **sp)
        if k == 0:
            t = cg.revcomp(t)
        qs.append(("cds%d" % k, q))
        ts.append(("gene%d" % k, t))
    return qs, ts


def run(tmp_path, env, extra=()):
    """A heuristic coding2genome run of the three CDS against the three targets on both binaries: (the reference's stdout,
    exonerate-gpu's stdout, its stderr)."""
    qs, ts = inputs()
    qf, tf = _write(tmp_path, qs, ts)
    args = ["-m", "coding2genome"] + REPORTS + list(extra) + [qf, tf]
    ref = subprocess.run([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                         env=dict(os.environ, C4GPU_VERBOSE="1", **env))
    assert ref.returncode == 0, ref.stderr.decode()[-800:]
    assert gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    return ref.stdout, gpu.stdout, gpu.stderr.decode()


def vulgars(out):
    return [l.split() for l in out.decode().splitlines() if l.startswith("vulgar:")]


@pytest.mark.parametrize("extra", [[], ["--bestn", "1"]], ids=["all", "bestn"])
def test_host_mode_is_byte_identical_and_every_pair_goes_through_the_seam(tmp_path, extra):
    ref, gpu, err = run(tmp_path, SWITCH, extra)
    vul = vulgars(ref)
    assert gpu == ref and len(vul) >= 3
    assert any("I" in f[10:] for f in vul)                                       # an intron in a vulgar line
    assert any("-" in (f[4], f[8]) for f in vul) and any((f[4], f[8]) == ("+", "+") for f in vul)      # both strands
    line = sdp_line(err)
    assert line and line[0] >= 3 and line[2] == line[0] and line[3] >= len(vul), err[-1500:]


def test_without_the_switch_nothing_moves(tmp_path):
    ref, gpu, err = run(tmp_path, HOST)
    assert gpu == ref and len(vulgars(ref)) >= 3
    assert sdp_line(err) is None and "c4gpu sdp:" not in err


def test_the_coding2coding_switch_alone_leaves_this_model_alone(tmp_path):
    ref, gpu, err = run(tmp_path, dict(HOST, C4GPU_CODON_SDP="1"))
    assert gpu == ref
    assert sdp_line(err) is None and "c4gpu sdp:" not in err
