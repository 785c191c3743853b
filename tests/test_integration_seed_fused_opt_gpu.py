"""The fused route of the word-scan seam (integration/c4gpu_seed.c, C4GPU_SEED_FUSED=1 with C4GPU_SEED_FUSED_OPT=1 beside it) under --softmaskquery, --softmasktarget
and --seedrepeat 2 with the device doing the work: one c4gpu_seed_extend_opt call per target, the alphabets' soft-mask flags and
the loader's seed_repeat handed over; the output is the reference's, byte for byte (inputs: tests/seed_fused_opt_dropin.py).  The
route's delivery code without a device: test_integration_seed_fused_opt_host.py."""
import os

import pytest

import seed_fused_opt_dropin as sd
from test_integration_bsdp_host import GPU_EXE, CPU_EXE

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                 reason="reference binaries are built in the build container (make -C integration)")]


@pytest.mark.parametrize("option", sd.OPTIONS, ids=lambda o: "".join(x.strip("-") for x in o))
@pytest.mark.parametrize("kind", sorted(sd.KINDS))
def test_fused_route_under_the_options_on_the_device_is_byte_identical(tmp_path, kind, option):
    ref, gpu, err = sd.run(tmp_path, kind, option, {"C4GPU_SEED_FUSED": "1", "C4GPU_SEED_FUSED_OPT": "1", "C4GPU_SEED_FACTOR": "0"})
    assert gpu == ref and ref.count(b"sugar:") >= 2
    targets, hits, extended, kept = sd.fused_line(err)
    assert targets > 0 and hits >= extended >= kept > 0
    assert "takes the scan and extension calls" not in err and "scanned on the CPU" not in err
    assert "c4gpu hsp:" not in err                      # no word hit went through the extension seam
