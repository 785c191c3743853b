#!/usr/bin/env python3
"""c4gpu_seed_extend_opt on soft-masked targets against the route such a target takes without it, alternated in one process (GPU).

  existing  what the drop-in does for a soft-masked target when the one-call seeder declines it: c4gpu_seed_scan (every word hit
            comes down, 8 B each) -> seeds and chain numbers on the host, as hsp_flush numbers them (here with numpy) ->
            c4gpu_hsp_extend_chains_masked (seeds, chains and horizons go up, one c4gpu_hsp and a dropped flag per word hit come
            down) -> threshold on the host
  opt       c4gpu_seed_extend_opt with mask_target = 1: the kept HSPs come down

Shapes: 64 and 256 cDNAs of 1 kb (5 % mutated pieces of the target) against DNA targets of 1 Mb and 10 Mb, of which about 40 % is
lower case in stretches of 200 to 2 000 bases (--softmasktarget yes: the scan string has column 0 there, the pairs carry the case).
Both routes are warmed, then timed in turn with wall time around calls that end in a synchronise; the results are compared HSP for
HSP before any time is reported.  Markdown on stdout.  (tools/bench_seed_fused.py: the unmasked call against its own predecessor.)"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import exonerate_amd as ex
from exonerate_amd import _abi
from bench_seed_fused import Runner, ptr


def shape_softmasked(n_queries, target_len):
    rng = np.random.default_rng(20261020 + n_queries + target_len // 1000)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    t = dna[rng.integers(0, 4, size=target_len)]
    queries = []
    for k in range(n_queries):
        p = int(rng.integers(0, len(t) - 1000))
        q = t[p:p + 1000].copy()
        hit = rng.random(1000) < 0.05
        q[hit] = dna[rng.integers(0, 4, size=int(hit.sum()))]
        queries.append(q.tobytes())
    low = np.zeros(target_len, dtype=bool)
    x = 0
    while x < target_len:                                     # upper-case and lower-case stretches in turn, about 60 : 40
        x += int(rng.integers(300, 3000))
        n = int(rng.integers(200, 2000))
        low[x:x + n] = True
        x += n
    column = np.zeros(256, dtype=np.uint8)
    for i, b in enumerate("ACGT"):
        column[ord(b)] = i + 1
    sym = column[t]
    sym[low] = 0                                              # Sequence_mask: a masked base is the wildcard, outside the automaton
    raw = t.copy()
    raw[low] += 32
    return dict(name="%d cDNAs of 1 kb x %d Mb soft-masked (%.0f %% lower case), dna2dna, words of 12" %
                (n_queries, target_len // 1000000, 100.0 * low.mean()), match=_abi.MATCH_DNA2DNA, queries=queries, target=raw.tobytes(),
                width=5, wordlen=12, column=column, strings=[np.ascontiguousarray(sym)], scale=1, offsets=[0], modifier=11, at=1,
                dropoff=30, threshold=75)


class MaskedRunner(Runner):
    def existing(self):
        sh, lib = self.sh, self.lib
        sym = sh["strings"][0]
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
        seeds = np.empty((len(hits), 3), dtype=np.int32)
        seeds[:, 0], seeds[:, 1], seeds[:, 2] = em[:, 0], em[:, 1], hits[:, 0] - sh["modifier"]
        if not len(seeds):
            return seeds, np.empty((0, 5), dtype=np.int32), np.empty(0, dtype=np.int64), 0
        qlen = self.qlen[seeds[:, 0]]
        section = np.fmod(seeds[:, 2].astype(np.int64) - seeds[:, 1].astype(np.int64) + qlen, qlen)
        assert (section >= 0).all()                           # (query and target advance 1: every seed has an entry)
        _, chain = np.unique(self.slot_base[seeds[:, 0]] + section, return_inverse=True)
        chain = np.ascontiguousarray(chain.astype(np.int32))
        n_chains = int(chain.max()) + 1
        horizon0 = np.zeros(n_chains, dtype=np.int32)
        out = np.empty((len(seeds), 5), dtype=np.int32)
        dropped = np.empty(len(seeds), dtype=np.int32)
        assert lib.c4gpu_hsp_extend_chains_masked(self.eng.ctx, self.params, sh["match"], self.pairs, len(self.pairs), sh["wordlen"],
                                                  sh["dropoff"], 0, 1, sh["threshold"], ptr(seeds, _abi.HspSeed), len(seeds),
                                                  ptr(chain, C.c_int32), n_chains, ptr(horizon0, C.c_int32), ptr(out, _abi.Hsp),
                                                  ptr(dropped, C.c_int32)) == 0, lib.c4gpu_last_error()
        keep = (out[:, 2] >= 0) & (dropped == 0) & (out[:, 3] >= sh["threshold"])
        return seeds, out[keep], np.nonzero(keep)[0], int((dropped != 0).sum())

    def fused(self):
        sh, lib = self.sh, self.lib
        sp = (C.c_char_p * 1)(sh["strings"][0].ctypes.data_as(C.c_char_p))
        sn = (C.c_int32 * 1)(len(sh["strings"][0]))
        so = (C.c_int32 * 1)(0)
        stats = _abi.SeedExtendStats()
        while True:
            out = np.empty(self.cap_kept, dtype=np.dtype([("seed", np.int64), ("pair", np.int32), ("hsp", np.int32, 5)]))
            assert lib.c4gpu_seed_extend_opt(self.eng.ctx, self.tab, self.params, sh["match"], self.pairs, len(self.pairs), sp, sn, 1,
                                             sh["scale"], so, sh["modifier"], sh["wordlen"], sh["dropoff"], sh["threshold"], 0, 1, 1,
                                             ptr(out, _abi.SeedHsp), self.cap_kept, C.byref(stats)) == 0, lib.c4gpu_last_error()
            if stats.n_kept <= self.cap_kept:
                break
            self.cap_kept = stats.n_kept
        return out[:stats.n_kept], stats


def measure(eng, sh, rounds):
    r = MaskedRunner(eng, sh)
    try:
        for _ in range(2):                                   # warm both: code objects, buffers, capacities
            seeds, old, old_at, n_dropped = r.existing()
            new, stats = r.fused()
        assert len(new) == len(old) and (new["seed"] == old_at).all() and (new["hsp"] == old).all(), "the two routes differ"
        t_old, t_new = [], []
        for _ in range(rounds):
            t0 = time.perf_counter(); r.existing(); t1 = time.perf_counter(); r.fused(); t2 = time.perf_counter()
            t_old.append((t1 - t0) * 1e3); t_new.append((t2 - t1) * 1e3)
        f = lambda t: "%.1f (%.1f - %.1f)" % (float(np.median(t)), min(t), max(t))
        print("| %s | %d | %d | %d | %d | %s | %s | %.2f |" % (sh["name"], stats.n_hits, stats.n_extended, n_dropped, stats.n_kept, f(t_old),
                                                               f(t_new), float(np.median(t_old)) / float(np.median(t_new))))
        sys.stdout.flush()
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--queries", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--megabases", type=int, nargs="*", default=[1, 10])
    a = ap.parse_args()
    eng = ex.Engine(0)
    print("| shape (per target) | word hits | extended | dropped | kept | scan + host replay + chains_masked ms, median (min - max) | "
          "seed_extend_opt ms, median (min - max) | ratio |")
    print("|---|---|---|---|---|---|---|---|")
    for mb in a.megabases:
        for n in a.queries:
            measure(eng, shape_softmasked(n, mb * 1000000), a.rounds)
    eng.close()


if __name__ == "__main__":
    main()
