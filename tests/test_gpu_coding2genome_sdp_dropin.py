"""The opt-in SDP seam of the drop-in binary for coding2genome (C4GPU_CODING2GENOME_SDP=1) with the device doing the work: a
heuristic run with --gappedextension yes whose SDP alignments come from c4gpu_sdp_batch (the boundary flavour of the sparse
wavefront with one ring per query advance, c4_sdp_wave.h); the output is the reference's, byte for byte.  The seam's host mode:
test_coding2genome_sdp_dropin_host.py."""
import os

import pytest

from test_coding2genome_sdp_dropin_host import run, vulgars, sdp_line, GPU_EXE, CPU_EXE

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                 reason="reference binaries are built in the build container (make -C integration)")]

DEVICE = {"C4GPU_CODING2GENOME_SDP": "1", "C4GPU_SEED_FACTOR": "0", "C4GPU_BATCH": "4096"}
NO_FALLBACK = ("SDP stays on the CPU", "using the CPU", "falls back", "scanned on the CPU", "HSP extensions of this scan on the CPU")


@pytest.mark.parametrize("extra", [[], ["--bestn", "1"]], ids=["all", "bestn"])
def test_runs_on_the_device_are_byte_identical(tmp_path, extra):
    ref, gpu, err = run(tmp_path, DEVICE, extra)
    vul = vulgars(ref)
    assert gpu == ref and len(vul) >= 3 and any("I" in f[10:] for f in vul)
    line = sdp_line(err)
    # every pair with HSPs went to the device and came back served (3 queries x 3 targets x 4 strand combinations at the most)
    assert line and 3 <= line[0] <= 36 and line[2] == line[0] and line[3] >= len(vul), err[-1500:]
    for text in NO_FALLBACK:
        assert text not in err, err[-1500:]
