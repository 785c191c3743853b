"""ctypes binding of build/libc4sdpcodonsim.so (tests/sdp_codon_sim.hip): the product's sparse SDP wavefront for
coding2coding (query advance up to 3: one ring per hop, three carried rows) -- its per-lane cell function, streams, walk and
host side -- driven by CPU loops.  TEST INFRASTRUCTURE, the sibling of sdp_sim_lib.py; never imported by exonerate_amd/."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib
from exonerate_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "build", "libc4sdpcodonsim.so")
SRC = [os.path.join(ROOT, "tests", "sdp_codon_sim.hip")] + [os.path.join(ROOT, "exonerate_amd", "csrc", f)
                                                            for f in ("c4_sdp_wave.h", "c4_sdp_host.h", "c4_viterbi_kernel.h")]
_lib = None


def load():
    global _lib
    if _lib is None:
        if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(x) for x in SRC):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--offload-host-only", "-DC4SDP_HOST_SIM", "-O1", "-std=c++17",
                                   "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                                   "-I" + os.path.join(ROOT, "exonerate_amd", "csrc"), SRC[0], "-o", SO,
                                   "-L" + os.path.join(ROOT, "exonerate_amd"), "-lc4gpu",
                                   "-Wl,-rpath," + os.path.join(ROOT, "exonerate_amd")])
        _abi.load()
        lib = C.CDLL(SO)
        lib.sdpcodonsim_pair.restype = C.c_int32
        lib.sdpcodonsim_pair.argtypes = [C.POINTER(_abi.Model), C.POINTER(_abi.Params), C.c_void_p, C.c_void_p,
                                         C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(_abi.Hsp), C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_abi.Alignment),
                                         C.POINTER(C.c_int64), C.c_int32]
        _lib = lib
    return _lib


def coded(params, s):
    """What ResidentSeqs builds for either sequence of a coding2coding batch (codon_kernel): at every position the matrix row of
    the residue the codon starting there encodes; the last two positions, and the padding, hold 0."""
    idx = np.frombuffer(bytes(params.submat_index), dtype=np.uint8)
    nt2d = np.frombuffer(bytes(params.nt2d), dtype=np.uint8).astype(np.int64)
    trans = np.frombuffer(bytes(params.trans), dtype=np.uint8)
    aa = np.frombuffer(bytes(params.aa), dtype=np.uint8)
    n = len(s)
    code = np.zeros(n + 64, dtype=np.uint8)
    if n >= 3:
        d = nt2d[np.frombuffer(s, dtype=np.uint8)]
        code[:n - 2] = idx[aa[trans[d[:-2] | (d[1:-1] << 4) | (d[2:] << 8)]]]
    assert code.max(initial=0) < 24
    return code


def sdp(model, params, q, t, hsps, query_advance=3, target_advance=3, dropoff=50, threshold=100, max_alignments=8,
        qid="qy", arena_chunks=2048):
    """(alignment dicts, wave steps executed): same contract as oracle_lib.sdp (single pass)."""
    lib = load()
    qcode, tcode = coded(params, q), coded(params, t)
    n = len(hsps)
    hs = (_abi.Hsp * max(1, n))(*[_abi.Hsp(*h) for h in hsps])
    out = (_abi.Alignment * max_alignments)()
    steps = C.c_int64(0)
    k = lib.sdpcodonsim_pair(model, params, qcode.ctypes.data, tcode.ctypes.data, q, len(q), t, len(t), hs, n,
                             query_advance, target_advance, dropoff, threshold, max_alignments, out, C.byref(steps), arena_chunks)
    assert k >= 0, "sdpcodonsim_pair failed: %d" % k
    res = []
    flib = _abi.load()
    for i in range(k):
        res.append(oracle_lib.alignment_to_dict(model, out[i], flib.c4gpu_alignment_format, qid, len(q), len(t)))
        flib.c4gpu_alignment_clear(out[i])
    return res, steps.value
