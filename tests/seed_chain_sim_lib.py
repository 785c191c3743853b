"""ctypes binding of build/libc4seedchainsim.so (tests/seed_chain_sim.hip): the product's step on one horizon entry
(hsp_entry_step, exonerate_amd/csrc/c4_hsp_extend.h) compiled for the host, in a CPU loop over a walk grouped by entry as
seed_chain_kernel takes it lane by lane.  TEST INFRASTRUCTURE beside hsp_sim_lib.py, whose coded and mask arrays it uses; never
imported by exonerate_amd/."""
import ctypes as C
import os
import subprocess

import numpy as np

import hsp_sim_lib
import hsp_codon_sim_lib
from exonerate_amd import _abi
from seed_fused_opt_cases import ADVANCE, entry_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "build", "libc4seedchainsim.so")
SRC = [os.path.join(ROOT, "tests", "seed_chain_sim.hip"), os.path.join(ROOT, "exonerate_amd", "csrc", "c4_hsp_extend.h")]
_lib = None


class HspJob(C.Structure):
    _fields_ = [("qoff", C.c_longlong), ("toff", C.c_longlong), ("qlen", C.c_int), ("tlen", C.c_int)]


def load():
    global _lib
    if _lib is None:
        if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(x) for x in SRC):
            os.makedirs(os.path.dirname(SO), exist_ok=True)
            subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "--offload-host-only", "-O1", "-std=c++17", "-shared",
                                   "-fPIC", "-I" + os.path.join(ROOT, "include"), SRC[0], "-o", SO])
        lib = C.CDLL(SO)
        lib.seedchainsim_walk.restype = C.c_int
        lib.seedchainsim_walk.argtypes = [C.c_void_p] * 4 + [C.POINTER(HspJob), C.c_void_p] + [C.c_int] * 6 + \
            [C.POINTER(_abi.HspSeed), C.c_int, C.c_void_p, C.c_int, C.POINTER(_abi.Hsp), C.c_void_p]
        _lib = lib
    return _lib


def walk(params, match, queries, target, calls, seedlen, dropoff, threshold, mask_query=False, mask_target=False, seed_repeat=1):
    """What replay_opt returns (kept HSPs with walk index and query, the counters), and the verdict per call, from the product's
    step: the queries' arrays behind each other in one buffer, the one target at offset 0, the entries numbered in order of first
    use."""
    aq, at = ADVANCE[match]
    if match == "codon2codon":
        sides = [hsp_codon_sim_lib.CodonPair(params, q, target, mask_query, mask_target) for q in queries]
    else:
        sides = [hsp_sim_lib.Pair(params, match, q, target, mask_query, mask_target) for q in queries]
    jobs, off = (HspJob * max(1, len(queries)))(), 0
    for i, p in enumerate(sides):
        jobs[i] = HspJob(off, 0, p.qlen, p.tlen)
        off += len(p.qcode)
    qcode = np.concatenate([p.qcode for p in sides])
    qmask = np.concatenate([p.qmask for p in sides]) if mask_query else None
    tcode, tmask, mat = sides[0].tcode, sides[0].tmask, sides[0].mat
    keys, entry = {}, []
    for qi, qs, ts in calls:
        e = entry_of(match, sides[qi].qlen, qs, ts)
        entry.append(-1 if e is None else keys.setdefault((qi,) + e, len(keys)))
    n = len(calls)
    seeds = (_abi.HspSeed * max(1, n))(*[_abi.HspSeed(qi, qs, ts) for qi, qs, ts in calls])
    ce = np.array(entry + [0], dtype=np.int32)
    out = (_abi.Hsp * max(1, n))()
    verdict = np.zeros(n + 1, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data if a is not None else None
    n_extended = load().seedchainsim_walk(ptr(qcode), ptr(tcode), ptr(qmask), ptr(tmask), jobs, ptr(mat), aq, at, seedlen, dropoff,
                                          threshold, seed_repeat, seeds, n, ce.ctypes.data, len(keys), out, verdict.ctypes.data)
    kept = [(k, calls[k][0], out[k].aslist()) for k in range(n) if verdict[k] == 2]
    stats = dict(n_hits=n, n_extended=n_extended, n_below=n_extended - len(kept), n_kept=len(kept))
    return kept, stats, [int(v) for v in verdict[:n]]
