"""The product's HSP extension routine (exonerate_amd/csrc/c4_hsp_extend.h, compiled for the host as tests/hsp_sim.hip)
with advances 3/3 and codon-row arrays on BOTH sides: what a FAM_UNGAPPED_CODON batch hands the kernels for
C4GPU_MATCH_CODON2CODON.  TEST INFRASTRUCTURE, beside hsp_sim_lib.py (whose library and soft-mask array it uses)."""
import numpy as np

import hsp_sim_lib
from exonerate_amd import _abi
from hsp_codon_cases import entry


def codon_rows(params, seq):
    """codon_kernel's array with numpy: per position the matrix row of the residue the codon starting there encodes; the last
    two positions (and the padding) 0."""
    idx = np.frombuffer(bytes(params.submat_index), dtype=np.uint8)
    nt2d = np.frombuffer(bytes(params.nt2d), dtype=np.uint8).astype(np.int64)
    trans = np.frombuffer(bytes(params.trans), dtype=np.uint8)
    aa = np.frombuffer(bytes(params.aa), dtype=np.uint8)
    s = np.frombuffer(seq, dtype=np.uint8)
    out = np.zeros(len(seq) + 64, dtype=np.uint8)
    if len(seq) >= 3:
        d = nt2d[s]
        out[:len(seq) - 2] = idx[aa[trans[d[:-2] | (d[1:-1] << 4) | (d[2:] << 8)]]]
    return out


class CodonPair(hsp_sim_lib.Pair):
    """One codon-vs-codon pair as a launch sees it."""

    def __init__(self, params, query, target, mask_query=False, mask_target=False):
        self.aq = self.at = 3
        q, t = query.encode(), target.encode()
        self.qlen, self.tlen = len(q), len(t)
        self.qcode, self.tcode = codon_rows(params, q), codon_rows(params, t)
        self.mat = np.frombuffer(bytes(params.protein_submat), dtype=np.int32).copy()
        assert self.mat.size == 24 * 24
        self.qmask = hsp_sim_lib.soft_mask(q, 3, "n") if mask_query else None
        self.tmask = hsp_sim_lib.soft_mask(t, 3, "n") if mask_target else None
        self.masked = bool(mask_query or mask_target)

    def walk(self, seedlen, dropoff, threshold, seeds):
        """The seeds in order under the horizon of a fresh set, the entries keyed in the reference's unsigned arithmetic."""
        keys, chain = {}, []
        for qs, ts in seeds:
            chain.append(keys.setdefault(entry(self.qlen, qs, ts), len(keys)))
        n = len(seeds)
        cs = (_abi.HspSeed * max(1, n))(*[_abi.HspSeed(0, qs, ts) for qs, ts in seeds])
        cc = np.array(chain + [0], dtype=np.int32)
        horizon = np.zeros(len(keys) + 1, dtype=np.int32)
        out = (_abi.Hsp * max(1, n))()
        dropped = np.zeros(n + 1, dtype=np.int32)
        hsp_sim_lib.load().hspsim_walk(*self._args(seedlen, dropoff, threshold), cs, n, cc.ctypes.data, horizon.ctypes.data, out,
                                       dropped.ctypes.data)
        return [None if out[k].length == -1 else (out[k].aslist(), int(dropped[k])) for k in range(n)]
