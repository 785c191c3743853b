"""ctypes binding of build/libc4hspsim.so (tests/hsp_sim.hip): the product's extension of one HSP seed and its horizon step
(exonerate_amd/csrc/c4_hsp_extend.h) compiled for the host.  TEST INFRASTRUCTURE: lets the build container (no GPU) hold the
routine the device kernels loop around to the reference's recorded HSPs; never imported by exonerate_amd/."""
import ctypes as C
import os
import subprocess

import numpy as np

import sdp_sim_lib
from exonerate_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "build", "libc4hspsim.so")
SRC = [os.path.join(ROOT, "tests", "hsp_sim.hip"), os.path.join(ROOT, "exonerate_amd", "csrc", "c4_hsp_extend.h")]
ADVANCE = {"dna2dna": (1, 1), "protein2protein": (1, 1), "protein2dna": (1, 3)}
_lib = None


def load():
    global _lib
    if _lib is None:
        if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(x) for x in SRC):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--offload-host-only", "-O1", "-std=c++17", "-shared",
                                   "-fPIC", "-I" + os.path.join(ROOT, "include"), SRC[0], "-o", SO])
        lib = C.CDLL(SO)
        pair = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 5
        lib.hspsim_seed.restype = C.c_int
        lib.hspsim_seed.argtypes = pair + [C.c_int, C.c_int, C.POINTER(_abi.Hsp)]
        lib.hspsim_walk.restype = None
        lib.hspsim_walk.argtypes = pair + [C.POINTER(_abi.HspSeed), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(_abi.Hsp), C.c_void_p]
        _lib = lib
    return _lib


def soft_mask(seq, advance, wild):
    """softmask_kernel's array with numpy: per position, is the strand position starting there masked -- a lower-case
    letter other than the wildcard, for a strand of advance 3 in any of its three bases; padded like the coded arrays."""
    a = np.frombuffer(seq, dtype=np.uint8)
    low = (a >= 97) & (a <= 122) & (a != ord(wild))
    m = np.zeros(len(seq) + 64, dtype=np.uint8)
    if advance == 3:
        if len(seq) >= 3:
            m[:len(seq) - 2] = low[:-2] | low[1:-1] | low[2:]
    else:
        m[:len(seq)] = low
    return m


class Pair:
    """One pair as a launch sees it: coded arrays (sdp_sim_lib.coded), matrix, and the mask arrays of the flagged sides.
    With no side flagged the plain routine runs, as the entry points have it."""

    def __init__(self, params, match, query, target, mask_query=False, mask_target=False):
        self.aq, self.at = ADVANCE[match]
        q, t = query.encode(), target.encode()
        self.qlen, self.tlen = len(q), len(t)
        self.qcode, self.tcode = sdp_sim_lib.coded(params, "protein2dna" if match == "protein2dna" else "affine", q, t)[:2]
        self.mat = np.frombuffer(bytes(params.dna_submat if match == "dna2dna" else params.protein_submat), dtype=np.int32).copy()
        assert self.mat.size == 24 * 24
        self.qmask = soft_mask(q, self.aq, "n" if match == "dna2dna" else "x") if mask_query else None
        self.tmask = soft_mask(t, self.at, "x" if match == "protein2protein" else "n") if mask_target else None
        self.masked = bool(mask_query or mask_target)

    def _args(self, seedlen, dropoff, threshold):
        ptr = lambda a: a.ctypes.data if a is not None else None
        return [int(self.masked), ptr(self.qcode), ptr(self.tcode), ptr(self.qmask), ptr(self.tmask), self.qlen, self.tlen,
                ptr(self.mat), self.aq, self.at, seedlen, dropoff, threshold]

    def seed(self, seedlen, dropoff, threshold, qs, ts):
        """([query_start, target_start, length, score, cobs], dropped) of one seed."""
        out = _abi.Hsp()
        dropped = load().hspsim_seed(*self._args(seedlen, dropoff, threshold), qs, ts, C.byref(out))
        return out.aslist(), dropped

    def walk(self, seedlen, dropoff, threshold, seeds):
        """The seeds (query_start, target_start) in order under the diagonal horizon of a fresh set: per seed None (skipped)
        or (hsp, dropped)."""
        keys, chain = {}, []
        for qs, ts in seeds:
            chain.append(keys.setdefault(((ts * self.aq - qs * self.at + self.qlen) % self.qlen, qs % self.aq, ts % self.at), len(keys)))
        n = len(seeds)
        cs = (_abi.HspSeed * max(1, n))(*[_abi.HspSeed(0, qs, ts) for qs, ts in seeds])
        cc = np.array(chain + [0], dtype=np.int32)
        horizon = np.zeros(len(keys) + 1, dtype=np.int32)
        out = (_abi.Hsp * max(1, n))()
        dropped = np.zeros(n + 1, dtype=np.int32)
        load().hspsim_walk(*self._args(seedlen, dropoff, threshold), cs, n, cc.ctypes.data, horizon.ctypes.data, out, dropped.ctypes.data)
        return [None if out[k].length == -1 else (out[k].aslist(), int(dropped[k])) for k in range(n)]
