#!/usr/bin/env python3
"""c4gpu_seed_extend against the sequence of calls it replaces, alternated in one process (GPU).

  existing  c4gpu_seed_scan per string (every word hit comes down, 8 B each) -> seeds and chain numbers on the host, as the
            drop-in's hsp_flush numbers them (one per (pair, section, target frame); here with numpy) -> c4gpu_hsp_extend_chains
            (seeds, chains and horizons go up, one c4gpu_hsp per word hit comes down) -> threshold on the host
  fused     c4gpu_seed_extend: the kept HSPs come down

Shapes: 1) 256 proteins of 300 aa against one 10 Mb target, three frames, protein2dna; 2) 4 096 cDNAs of 1 kb against a 1 Mb
target, dna2dna.  The word tables hold the queries' exact words (the drop-in's protein tables also hold word neighbourhoods:
many more hits per position; --proteinwordlen 5 is a stand-in for that density).  Both routes are warmed, then timed in turn
with wall time around calls that end in a synchronise; the results are compared.  Markdown on stdout."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import exonerate_amd as ex
from exonerate_amd import _abi, workloads

AA = "ARNDCQEGHILKMFPSTWYV"
TABLE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def word_table(queries, wordlen, column, width):
    """codes (uint64, one per distinct word), emit_first (int32), emits (pair, query position) grouped by word."""
    codes, pair, pos = [], [], []
    for k, q in enumerate(queries):
        col = column[np.frombuffer(q, dtype=np.uint8)].astype(np.uint64)
        n = len(col) - wordlen + 1
        if n <= 0:
            continue
        code, ok = np.zeros(n, dtype=np.uint64), np.ones(n, dtype=bool)
        for w in range(wordlen):
            code = code * np.uint64(width) + col[w:w + n]
            ok &= col[w:w + n] != 0
        codes.append(code[ok]); pair.append(np.full(int(ok.sum()), k, dtype=np.int32)); pos.append(np.nonzero(ok)[0].astype(np.int32))
    codes, pair, pos = np.concatenate(codes), np.concatenate(pair), np.concatenate(pos)
    order = np.argsort(codes, kind="stable")
    uniq, first = np.unique(codes[order], return_index=True)
    emit_first = np.append(first, len(order)).astype(np.int32)
    emits = np.ascontiguousarray(np.stack([pair[order], pos[order]], axis=1).astype(np.int32))
    return np.ascontiguousarray(uniq), emit_first, emits


def shape_protein(n, wordlen):
    proteins, contig, _ = workloads.protein_vs_contig(n, 300, 10000000, seed=20260935, introns=True)
    column = np.zeros(256, dtype=np.uint8)
    for i, a in enumerate(AA):
        column[ord(a)] = i + 1
    base = np.full(256, 64, dtype=np.int64)
    for i, b in enumerate("TCAG"):
        base[ord(b)] = i
    t = base[np.frombuffer(contig, dtype=np.uint8)]
    aa_col = np.array([column[ord(a)] for a in TABLE] + [0], dtype=np.uint8)
    strings = []
    for f in range(3):
        m = (len(t) - f) // 3
        c = t[f:f + 3 * m].reshape(m, 3)
        idx = np.where((c < 4).all(axis=1), c[:, 0] * 16 + c[:, 1] * 4 + c[:, 2], 64)
        strings.append(np.ascontiguousarray(aa_col[idx]))
    return dict(name="%d proteins of 300 aa x 10 Mb, three frames, protein2dna, words of %d" % (n, wordlen), match=_abi.MATCH_PROTEIN2DNA,
                queries=proteins, target=contig, width=21, wordlen=wordlen, column=column, strings=strings, scale=3, offsets=[0, 1, 2],
                modifier=wordlen * 3 - 3, at=3, dropoff=20, threshold=30)


def shape_dna(n):
    rng = np.random.default_rng(20260936)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    t = dna[rng.integers(0, 4, size=1000000)]
    queries = []
    for k in range(n):
        p = int(rng.integers(0, len(t) - 1000))
        q = t[p:p + 1000].copy()
        hit = rng.random(1000) < 0.05
        q[hit] = dna[rng.integers(0, 4, size=int(hit.sum()))]
        queries.append(q.tobytes())
    column = np.zeros(256, dtype=np.uint8)
    for i, b in enumerate("ACGT"):
        column[ord(b)] = i + 1
    return dict(name="%d cDNAs of 1 kb x 1 Mb, dna2dna, words of 12" % n, match=_abi.MATCH_DNA2DNA, queries=queries, target=t.tobytes(),
                width=5, wordlen=12, column=column, strings=[np.ascontiguousarray(column[t])], scale=1, offsets=[0], modifier=11, at=1,
                dropoff=30, threshold=75)


class Runner:
    def __init__(self, eng, sh):
        self.eng, self.sh, self.lib = eng, sh, _abi.load()
        self.params = ex.default_params()
        self.codes, self.emit_first, self.emits = word_table(sh["queries"], sh["wordlen"], sh["column"], sh["width"])
        self.tab = self.lib.c4gpu_wordtab_create(eng.ctx, sh["width"], sh["wordlen"], ptr(self.codes, C.c_uint64), ptr(self.emit_first, C.c_int32),
                                                 len(self.codes))
        assert self.tab, self.lib.c4gpu_last_error()
        assert self.lib.c4gpu_wordtab_set_emissions(self.tab, ptr(self.emits, _abi.SeedEmit), len(self.emits)) == 0
        n = len(sh["queries"])
        self.pairs = (_abi.Pair * n)()
        for i, q in enumerate(sh["queries"]):
            self.pairs[i].query, self.pairs[i].query_len, self.pairs[i].target, self.pairs[i].target_len = q, len(q), sh["target"], len(sh["target"])
        self.qlen = np.array([len(q) for q in sh["queries"]], dtype=np.int64)
        self.slot_base = np.concatenate([[0], np.cumsum(self.qlen * sh["at"])])
        self.cap_hits, self.cap_kept = 1 << 16, 1 << 12

    def existing(self):
        sh, lib = self.sh, self.lib
        seeds = []
        for s, sym in enumerate(sh["strings"]):
            n_hits = C.c_int64(0)
            while True:
                hits = np.empty((self.cap_hits, 2), dtype=np.int32)
                assert lib.c4gpu_seed_scan(self.eng.ctx, self.tab, sym.ctypes.data_as(C.c_char_p), len(sym), hits.ctypes.data, self.cap_hits,
                                           C.byref(n_hits)) == 0
                if n_hits.value <= self.cap_hits:
                    break
                self.cap_hits = n_hits.value
            hits = hits[:n_hits.value]
            em = self.emits[hits[:, 1]]
            sd = np.empty((len(hits), 3), dtype=np.int32)
            sd[:, 0], sd[:, 1], sd[:, 2] = em[:, 0], em[:, 1], hits[:, 0] * sh["scale"] + sh["offsets"][s] - sh["modifier"]
            seeds.append(sd)
        seeds = np.ascontiguousarray(np.concatenate(seeds))
        if not len(seeds):
            return seeds, np.empty((0, 5), dtype=np.int32), 0
        at, qlen = sh["at"], self.qlen[seeds[:, 0]]
        diag = seeds[:, 2].astype(np.int64) - seeds[:, 1].astype(np.int64) * at
        section = np.fmod(diag + qlen, qlen)                                   # C's remainder
        slot = np.where(section >= 0, self.slot_base[seeds[:, 0]] + section * at + seeds[:, 2] % at,
                        self.slot_base[-1] + np.arange(len(seeds)))            # no entry: a chain of its own
        _, chain = np.unique(slot, return_inverse=True)
        chain = np.ascontiguousarray(chain.astype(np.int32))
        n_chains = int(chain.max()) + 1
        horizon0 = np.zeros(n_chains, dtype=np.int32)
        horizon0[chain[section < 0]] = -2 ** 31
        out = np.empty((len(seeds), 5), dtype=np.int32)
        assert lib.c4gpu_hsp_extend_chains(self.eng.ctx, self.params, sh["match"], self.pairs, len(self.pairs), sh["wordlen"], sh["dropoff"],
                                           ptr(seeds, _abi.HspSeed), len(seeds), ptr(chain, C.c_int32), n_chains, ptr(horizon0, C.c_int32),
                                           ptr(out, _abi.Hsp)) == 0, lib.c4gpu_last_error()
        keep = (out[:, 2] >= 0) & (out[:, 3] >= sh["threshold"])
        return seeds, out[keep], np.nonzero(keep)[0]

    def fused(self):
        sh, lib = self.sh, self.lib
        sp = (C.c_char_p * len(sh["strings"]))(*[s.ctypes.data_as(C.c_char_p) for s in sh["strings"]])
        sn = (C.c_int32 * len(sh["strings"]))(*[len(s) for s in sh["strings"]])
        so = (C.c_int32 * len(sh["strings"]))(*sh["offsets"])
        stats = _abi.SeedExtendStats()
        while True:
            out = np.empty(self.cap_kept, dtype=np.dtype([("seed", np.int64), ("pair", np.int32), ("hsp", np.int32, 5)]))
            assert out.itemsize == C.sizeof(_abi.SeedHsp)
            assert lib.c4gpu_seed_extend(self.eng.ctx, self.tab, self.params, sh["match"], self.pairs, len(self.pairs), sp, sn, len(sh["strings"]),
                                         sh["scale"], so, sh["modifier"], sh["wordlen"], sh["dropoff"], sh["threshold"],
                                         ptr(out, _abi.SeedHsp), self.cap_kept, C.byref(stats)) == 0, lib.c4gpu_last_error()
            if stats.n_kept <= self.cap_kept:
                break
            self.cap_kept = stats.n_kept
        return out[:stats.n_kept], stats

    def close(self):
        self.lib.c4gpu_wordtab_destroy(self.tab)


def measure(eng, sh, rounds):
    r = Runner(eng, sh)
    try:
        for _ in range(2):                                   # warm both: code objects, buffers, capacities
            seeds, old, old_at = r.existing()
            new, stats = r.fused()
        assert len(new) == len(old) and (new["seed"] == old_at).all() and (new["hsp"] == old).all(), "the two routes differ"
        t_old, t_new = [], []
        for _ in range(rounds):
            t0 = time.perf_counter(); r.existing(); t1 = time.perf_counter(); r.fused(); t2 = time.perf_counter()
            t_old.append((t1 - t0) * 1e3); t_new.append((t2 - t1) * 1e3)
        f = lambda t: "%.1f (%.1f - %.1f)" % (float(np.median(t)), min(t), max(t))
        print("| %s | %d | %d | %d | %s | %s | %.2f |" % (sh["name"], stats.n_hits, stats.n_extended, stats.n_kept, f(t_old), f(t_new),
                                                          float(np.median(t_old)) / float(np.median(t_new))))
        sys.stdout.flush()
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--proteins", type=int, default=256)
    ap.add_argument("--cdnas", type=int, default=4096)
    ap.add_argument("--proteinwordlen", type=int, nargs="*", default=[6, 5])
    a = ap.parse_args()
    eng = ex.Engine(0)
    print("| shape | word hits | extended | kept | existing calls ms, median (min - max) | seed_extend ms, median (min - max) | ratio |")
    print("|---|---|---|---|---|---|---|")
    for w in a.proteinwordlen:
        measure(eng, shape_protein(a.proteins, w), a.rounds)
    measure(eng, shape_dna(a.cdnas), a.rounds)
    eng.close()


if __name__ == "__main__":
    main()
