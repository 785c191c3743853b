"""The opt-in fused route of the word-scan seam (integration/c4gpu_seed.c, C4GPU_SEED_FUSED=1) with the device doing the
work: one c4gpu_seed_extend call per target in place of scan, hit download, chain numbering, seed upload, extension and replay;
the output is the reference's, byte for byte.  The route's delivery code without a device: test_integration_seed_fused_host.py."""
import os
import re

import pytest

from test_integration_bsdp_host import run_pair, GPU_EXE, CPU_EXE

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                 reason="reference binaries are built in the build container (make -C integration)")]


@pytest.mark.parametrize("model,extra", [("affine:local", ["--gappedextension", "yes"]), ("protein2genome", ["--gappedextension", "yes"])])
def test_fused_route_on_the_device_is_byte_identical(tmp_path, model, extra):
    ref, gpu, err = run_pair(tmp_path, model, extra, {"C4GPU_SEED_FUSED": "1", "C4GPU_SEED_FACTOR": "0"}, n=8, seed=41)
    assert gpu == ref and ref.count(b"vulgar:") >= 4
    m = re.search(r"c4gpu seed fused: (\d+) targets through c4gpu_seed_extend: (\d+) word hits, (\d+) extensions, (\d+) HSPs kept", err)
    assert m, err[-1500:]
    targets, hits, extended, kept = [int(x) for x in m.groups()]
    assert targets > 0 and hits > 100 and hits > extended >= kept > 0
    assert "takes the scan and extension calls" not in err and "scanned on the CPU" not in err
    assert "c4gpu hsp:" not in err                      # no word hit went through the extension seam
