"""The opt-in SDP seam of the drop-in binary for coding2coding (C4GPU_CODON_SDP=1: a heuristic run with --gappedextension yes,
the default), checked WITHOUT a device: with C4GPU_SDP_HOST=1 the alignments behind the seam are the reference's own
SDP_Pair_next_path, so the seam's own work -- letting the one wide model with SDP passes through, gathering the comparison's codon
HSPs (advances 3/3), batching, the replay in submission order -- is exercised byte for byte against the unmodified reference.
Without the switch nothing moves.  The device route: test_gpu_codon_sdp_dropin.py."""
import os
import re
import subprocess

import pytest

from test_gpu_codon_dropin import _inputs, _write, GPU_EXE, CPU_EXE, REPORTS

pytestmark = pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                reason="reference binaries are built in the build container (make -C integration)")

HOST = {"C4GPU_SDP_HOST": "1", "C4GPU_HSP_HOST": "1", "C4GPU_SEED_HOST": "1", "C4GPU_BSDP_HOST": "1", "C4GPU_SEED_FACTOR": "0",
        "C4GPU_BATCH": "4096"}
SWITCH = dict(HOST, C4GPU_CODON_SDP="1")


def sdp_line(err):
    """(pairs, flushes, pairs served, alignments) of the seam's summary, or None when it served nothing."""
    m = re.search(r"c4gpu sdp: (\d+) pairs in (\d+) flush\(es\): (\d+) served from device batches \((\d+) alignments\)", err)
    return [int(x) for x in m.groups()] if m else None


def run(tmp_path, env, extra=(), reverse=True):
    """A heuristic coding2coding run of three homologous pairs (one target reverse-complemented: both strands) on both binaries:
    (the reference's stdout, exonerate-gpu's stdout, its stderr)."""
    qs, ts = _inputs(5, 3, reverse=reverse, lo=60, hi=90)
    qf, tf = _write(tmp_path, qs, ts)
    args = ["-m", "coding2coding"] + REPORTS + list(extra) + [qf, tf]
    ref = subprocess.run([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                         env=dict(os.environ, C4GPU_VERBOSE="1", **env))
    assert ref.returncode == 0, ref.stderr.decode()[-800:]
    assert gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    return ref.stdout, gpu.stdout, gpu.stderr.decode()


@pytest.mark.parametrize("extra", [[], ["--bestn", "1"]], ids=["all", "bestn"])
def test_host_mode_is_byte_identical_and_every_pair_goes_through_the_seam(tmp_path, extra):
    ref, gpu, err = run(tmp_path, SWITCH, extra)
    assert gpu == ref and ref.count(b"vulgar:") >= 3
    vul = [l.split() for l in ref.decode().splitlines() if l.startswith("vulgar:")]
    assert any("-" in (f[4], f[8]) for f in vul) and any((f[4], f[8]) == ("+", "+") for f in vul)      # both strands
    line = sdp_line(err)
    assert line and line[0] >= 3 and line[2] == line[0] and line[3] >= len(vul), err[-1500:]


def test_host_mode_with_the_codon_seeding_seams(tmp_path):
    ref, gpu, err = run(tmp_path, dict(SWITCH, C4GPU_CODON_SEED="1"))
    assert gpu == ref and ref.count(b"vulgar:") >= 3
    line = sdp_line(err)
    assert line and line[2] == line[0] >= 3
    assert "c4gpu hsp:" in err                               # the extension seam served the codon sets the SDP seam then read


def test_without_the_switch_nothing_moves(tmp_path):
    ref, gpu, err = run(tmp_path, HOST)
    assert gpu == ref
    assert sdp_line(err) is None and "c4gpu sdp:" not in err


def test_the_switch_leaves_ungapped_trans_alone(tmp_path):
    """ungapped:trans has no SDP in the reference (its alignments are its HSPs): the switch changes nothing there."""
    qs, ts = _inputs(5, 3, lo=60, hi=90)
    qf, tf = _write(tmp_path, qs, ts)
    args = ["-m", "ungapped:trans", "--score", "30"] + REPORTS + [qf, tf]
    ref = subprocess.run([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                         env=dict(os.environ, C4GPU_VERBOSE="1", **SWITCH))
    assert ref.returncode == 0 and gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    assert gpu.stdout == ref.stdout and "c4gpu sdp:" not in gpu.stderr.decode()
