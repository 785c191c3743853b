"""ctypes binding of build/libc4sdpc2gsim.so (tests/sdp_c2g_sim.hip): the product's sparse SDP wavefront for coding2genome
(the boundary flavour at a query advance of up to 3: one ring per hop with its shadow word, three carried rows, mirrored
boundary records, span stores) -- its per-lane cell function, streams, walk and host side -- driven by CPU loops.
TEST INFRASTRUCTURE, the sibling of sdp_sim_lib.py and sdp_codon_sim_lib.py; never imported by exonerate_amd/."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib
import sdp_codon_sim_lib
from exonerate_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "build", "libc4sdpc2gsim.so")
SRC = [os.path.join(ROOT, "tests", "sdp_c2g_sim.hip")] + [os.path.join(ROOT, "exonerate_amd", "csrc", f)
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
        lib.sdpc2gsim_pair.restype = C.c_int32
        lib.sdpc2gsim_pair.argtypes = [C.POINTER(_abi.Model), C.POINTER(_abi.Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(_abi.Hsp), C.c_int32,
                                       C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_abi.Alignment),
                                       C.POINTER(C.c_int64), C.c_int32]
        _lib = lib
    return _lib


def coded(params, q, t):
    """What ResidentSeqs builds for a coding2genome batch: codon row codes by position on both axes (codon_kernel), the four
    splice arrays (splice_kernel; here the oracle's restatement) with a stride of len(t) + 64, the base masks (tn4_kernel)."""
    qcode, tcode = sdp_codon_sim_lib.coded(params, q), sdp_codon_sim_lib.coded(params, t)
    n, pad = len(t), 64
    ss = np.zeros((4, n + pad), dtype=np.int32)
    lib = oracle_lib.load()
    for k in range(4):
        buf = (C.c_int32 * max(1, n))()
        lib.oracle_splice_predict(C.byref(params.splice[k]), t, n, buf)
        ss[k, :n] = np.frombuffer(buf, dtype=np.int32)[:n]
    nt2d = np.frombuffer(bytes(params.nt2d), dtype=np.uint8).astype(np.int64)
    d = nt2d[np.frombuffer(t, dtype=np.uint8)]
    v = np.zeros(n, dtype=np.int64)
    for s in range(4):
        v[s:] |= d[:n - s] << (4 * s)
    tn4 = np.zeros(n + pad, dtype=np.uint16)
    tn4[:n] = v.astype(np.uint16)
    return qcode, tcode, ss, tn4


def sdp(model, params, q, t, hsps, query_advance=1, target_advance=1, dropoff=50, threshold=100, max_alignments=8,
        qid="qy", arena_chunks=2048):
    """(alignment dicts, wave steps executed): same contract as oracle_lib.sdp (single pass)."""
    lib = load()
    qcode, tcode, ss, tn4 = coded(params, q, t)
    n = len(hsps)
    hs = (_abi.Hsp * max(1, n))(*[_abi.Hsp(*h) for h in hsps])
    out = (_abi.Alignment * max_alignments)()
    steps = C.c_int64(0)
    k = lib.sdpc2gsim_pair(model, params, qcode.ctypes.data, tcode.ctypes.data, ss.ctypes.data, tn4.ctypes.data,
                           q, len(q), t, len(t), hs, n, query_advance, target_advance, dropoff, threshold, max_alignments, out,
                           C.byref(steps), arena_chunks)
    assert k >= 0, "sdpc2gsim_pair failed: %d" % k
    res = []
    flib = _abi.load()
    for i in range(k):
        res.append(oracle_lib.alignment_to_dict(model, out[i], flib.c4gpu_alignment_format, qid, len(q), len(t)))
        flib.c4gpu_alignment_clear(out[i])
    return res, steps.value
