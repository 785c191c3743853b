"""The fused route of the word-scan seam (integration/c4gpu_seed.c, C4GPU_SEED_FUSED=1 with C4GPU_SEED_FUSED_OPT=1 beside it)
under --softmaskquery, --softmasktarget and --seedrepeat 2, checked WITHOUT a device: with C4GPU_SEED_HOST=1 the kept HSPs come from the reference's own HSPset_seed_hsp on
scratch sets and go through the route's own delivery.  Every run is byte for byte the unmodified reference, takes the fused route
for its targets, and the option decides what the reference prints (inputs: tests/seed_fused_opt_dropin.py).  The device route:
test_integration_seed_fused_opt_gpu.py."""
import os

import pytest

import seed_fused_opt_dropin as sd
from test_integration_bsdp_host import GPU_EXE, CPU_EXE
from test_integration_seed_fused_host import FUSED

pytestmark = pytest.mark.skipif(not (os.path.exists(GPU_EXE) and os.path.exists(CPU_EXE)),
                                reason="reference binaries are built in the build container (make -C integration)")


@pytest.mark.parametrize("option", sd.OPTIONS, ids=lambda o: "".join(x.strip("-") for x in o))
@pytest.mark.parametrize("kind", sorted(sd.KINDS))
def test_fused_route_under_the_options_is_byte_identical_with_host_sets(tmp_path, kind, option):
    ref, gpu, err = sd.run(tmp_path, kind, option, dict(FUSED, C4GPU_SEED_FUSED_OPT="1"))
    assert gpu == ref and ref.count(b"sugar:") >= 2
    targets, hits, extended, kept = sd.fused_line(err)
    assert targets > 0 and hits >= extended >= kept > 0
    assert "takes the scan and extension calls" not in err
    assert ref != sd.run(tmp_path, kind, None, None)                    # the option decides what the reference prints


@pytest.mark.parametrize("option", [sd.OPTIONS[1], sd.OPTIONS[3]], ids=lambda o: "".join(x.strip("-") for x in o))
def test_without_the_second_switch_such_runs_keep_the_other_route(tmp_path, option):
    """C4GPU_SEED_FUSED=1 alone: a soft-masked query or a repeat leaves the targets to the scan and extension calls, as before
    (a soft-masked target: test_integration_seed_fused_host.py)."""
    ref, gpu, err = sd.run(tmp_path, "dna", option, FUSED)
    assert gpu == ref and sd.fused_line(err)[0] == 0
