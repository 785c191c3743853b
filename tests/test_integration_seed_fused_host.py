"""The opt-in fused route of the word-scan seam (integration/c4gpu_seed.c, C4GPU_SEED_FUSED=1), checked WITHOUT a device:
with C4GPU_SEED_HOST=1 the kept HSPs come from the reference's own HSPset_seed_hsp on one scratch set per query, fed the host
scan's seeds in order, and go through the route's own delivery (Comparison on first use, HSPset_add_known_hsp) -- byte for byte
the unmodified reference, and byte for byte the same run without the switch.  The device route: test_integration_seed_fused_gpu.py."""
import re

import pytest

from test_integration_bsdp_host import run_pair, GPU_EXE, CPU_EXE
import os

pytestmark = pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                reason="reference binaries are built in the build container (make -C integration)")

HOST = {"C4GPU_SEED_HOST": "1", "C4GPU_HSP_HOST": "1", "C4GPU_SDP_HOST": "1", "C4GPU_BSDP_HOST": "1", "C4GPU_SEED_FACTOR": "0"}
FUSED = dict(HOST, C4GPU_SEED_FUSED="1")


def fused_line(err):
    m = re.search(r"c4gpu seed fused: (\d+) targets through c4gpu_seed_extend: (\d+) word hits, (\d+) extensions, (\d+) HSPs kept", err)
    assert m, err[-1500:]
    return [int(x) for x in m.groups()]


@pytest.mark.parametrize("model,extra", [
    ("affine:local", ["--gappedextension", "yes"]), ("protein2dna", []), ("protein2genome", ["--gappedextension", "yes"]),
    ("affine:local", ["--forcefsm", "compact", "--gappedextension", "yes"]), ("est2genome", ["--dnawordlen", "9"]),
    ("est2genome", ["--fsmmemory", "1"]), ("protein2genome", ["--hspfilter", "3"]),
])
def test_fused_route_is_byte_identical_with_host_sets(tmp_path, model, extra):
    ref, gpu, err = run_pair(tmp_path, model, extra, FUSED, n=6, seed=31)
    assert gpu == ref and ref.count(b"vulgar:") >= 3
    targets, hits, extended, kept = fused_line(err)
    assert targets > 0 and hits > 100 and hits > extended >= kept > 0
    assert "takes the scan and extension calls" not in err
    _, plain, err2 = run_pair(tmp_path, model, extra, HOST, n=6, seed=31)
    assert plain == gpu and "c4gpu seed fused" not in err2          # the switch is off by default


def test_softmasked_targets_keep_the_existing_route(tmp_path):
    ref, gpu, err = run_pair(tmp_path, "affine:local", ["--gappedextension", "yes", "--softmasktarget", "yes"], FUSED, n=6, seed=31)
    assert gpu == ref and ref.count(b"vulgar:") >= 3
    assert fused_line(err)[0] == 0
    assert re.search(r"c4gpu seed: (\d+) targets walked", err)


def test_check_modes_keep_the_existing_route(tmp_path):
    ref, gpu, err = run_pair(tmp_path, "est2genome", [], dict(FUSED, C4GPU_SEED_CHECK="1"), n=6, seed=31)
    assert gpu == ref and fused_line(err)[0] == 0 and "every seed equal to the reference's own walk" in err


def test_comparisons_are_reported_in_the_order_of_first_hits(tmp_path):
    """Many proteins against ONE contig: chance hits that are skipped or fall below the threshold come before most queries'
    first kept HSP, and the reference creates (and later reports) a query's Comparison at its first hit, kept or not."""
    import subprocess
    from exonerate_amd import workloads
    proteins, contig, _ = workloads.protein_vs_contig(24, 300, 150000, seed=20260935, introns=True)
    qf, tf = str(tmp_path / "q.fa"), str(tmp_path / "t.fa")
    with open(qf, "w") as f:
        f.write("".join(">p%d\n%s\n" % (i, p.decode()) for i, p in enumerate(proteins)))
    with open(tf, "w") as f:
        f.write(">chr\n%s\n" % contig.decode())
    args = ["-m", "protein2genome", "--showalignment", "no", "--showvulgar", "yes", "-V", "0", qf, tf]
    ref = subprocess.run([CPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    gpu = subprocess.run([GPU_EXE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                         env=dict(os.environ, C4GPU_VERBOSE="1", **FUSED))
    assert ref.returncode == 0 and gpu.returncode == 0, gpu.stderr.decode()[-1500:]
    assert gpu.stdout == ref.stdout and ref.stdout.count(b"vulgar:") >= 20
    assert fused_line(gpu.stderr.decode())[0] > 0
    order = [l.split()[1] for l in ref.stdout.decode().splitlines() if l.startswith("vulgar:")]
    assert order != sorted(order, key=lambda n: int(n[1:]))
