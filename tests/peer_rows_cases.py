"""Shared cases of the row-wise peer-lookup tests (tests/test_peer_rows_cpu.py,
tests/test_peer_rows_gpu.py): three stores in one process standing in for
three ranks (tests/peer_fp8_cases.py builds two), holding the same logical
tables three ways - cut into row ranges (the descriptor under test, seen from
any rank), placed whole (the table-wise descriptor the merged kernels read) and
concatenated into one local store - as e4m3 codes with per-table power-of-two
scales and as their exact bf16 dequantisation.

Tables: 4099 rows each (an uneven split over three ranks: 1367 / 1366 / 1366);
with T >= 2 the LAST table has 2 rows, so rank 2's range of it is empty (the
fused kernel takes at most 31 tables, so the small table is one of the T, not
an extra one). ``mixed``: every third table (t % 3 == 0) is placed whole on
one store - the degenerate ranges of a mixed plan."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peer_fp8_cases as pc  # noqa: E402

from distributed_tf_serving_amd.parallel.dist import split_rows  # noqa: E402
from distributed_tf_serving_amd.parallel.hot_cache import PeerTables  # noqa: E402

F8 = torch.float8_e4m3fn
S = 3
ROWS = 4099
SMALL = 2
PAD = (5, 0, 11)  # rows of other data in front of each store: the range offsets differ per rank


def table_rows(T: int):
    return [ROWS] * (T - 1) + [SMALL if T > 1 else ROWS]


class RowStores:
    def __init__(self, T: int, gen: torch.Generator, mixed: bool = False):
        self.T, self.mixed = T, mixed
        self.rows = table_rows(T)
        self.scale = pc.table_scales(T)
        self.codes = [pc.random_codes(n, gen) for n in self.rows]  # the logical tables
        self.deq = []
        for t, c in enumerate(self.codes):
            v = c.float() * self.scale[t]
            assert torch.equal(v.to(torch.bfloat16).float(), v)  # code x power of two is a bf16 value
            self.deq.append(v.to(torch.bfloat16))
        # ---- (a) row ranges: ranges[t][r] = (lo, n, store offset)
        fill = list(PAD)
        self.ranges, self.whole = [], {}
        for t, n in enumerate(self.rows):
            if mixed and t % 3 == 0:
                o = (t // 3) % S
                self.whole[t] = o
                rr = [(0, n) if r == o else (0 if r < o else n, 0) for r in range(S)]
            else:
                rr = split_rows(n, S)
            self.ranges.append([(lo, k, fill[r] if k else 0) for r, (lo, k) in enumerate(rr)])
            for r, (_, k) in enumerate(rr):
                fill[r] += k
        self.row_codes = [self._store(self.codes, r, fill[r], gen) for r in range(S)]
        self.row_deq = [self._deq_store(s, r) for r, s in enumerate(self.row_codes)]
        # ---- (b) the same tables placed whole: table t on store t % 3
        self.tw_owner = [t % S for t in range(T)]
        self.tw_off, used = [], [0] * S
        for t, n in enumerate(self.rows):
            self.tw_off.append(used[t % S])
            used[t % S] += n
        self.tw_codes = [torch.cat([self.codes[t].view(torch.uint8) for t in range(T) if t % S == r]
                                   + [torch.zeros(1, 64, dtype=torch.uint8)]).view(F8) for r in range(S)]
        self.tw_deq = [torch.cat([self.deq[t] for t in range(T) if t % S == r]
                                 + [torch.zeros(1, 64, dtype=torch.bfloat16)]) for r in range(S)]

    def _store(self, tables, r, total, gen):
        out = pc.random_codes(max(1, total), gen).view(torch.uint8)  # the pad rows hold other data
        for t, rr in enumerate(self.ranges):
            lo, n, off = rr[r]
            out[off:off + n] = tables[t].view(torch.uint8)[lo:lo + n]
        return out.view(F8)

    def _deq_store(self, store, r):
        out = torch.zeros(store.shape, dtype=torch.bfloat16)
        for t, rr in enumerate(self.ranges):
            lo, n, off = rr[r]
            out[off:off + n] = self.deq[t][lo:lo + n]
        return out

    @staticmethod
    def _split(stores, chunk_shift, dev):
        stores = [s.to(dev) for s in stores]
        if chunk_shift is not None:  # chunks = views of the store; the kernels only see chunk addresses
            stores = [list(torch.split(s, 1 << chunk_shift)) for s in stores]
        return stores

    def peer_rows(self, rank: int, fp8: bool, chunk_shift=None, dev="cpu") -> PeerTables:
        """(a) the row-wise descriptor as rank `rank` sees it."""
        return PeerTables(self._split(self.row_codes if fp8 else self.row_deq, chunk_shift, dev), None, None,
                          self.rows, rank=rank, chunk_shift=chunk_shift, scale=self.scale if fp8 else None,
                          ranges=self.ranges)

    def peer_tables(self, rank: int, fp8: bool, chunk_shift=None, dev="cpu") -> PeerTables:
        """(b) the table-wise descriptor over stores holding the same rows."""
        return PeerTables(self._split(self.tw_codes if fp8 else self.tw_deq, chunk_shift, dev), self.tw_owner,
                          self.tw_off, self.rows, rank=rank, chunk_shift=chunk_shift,
                          scale=self.scale if fp8 else None)

    def local(self, fp8: bool):
        """(c) every table in one store: (store, modulo_f, offset_f)."""
        store = torch.cat([c.view(torch.uint8) for c in self.codes]).view(F8) if fp8 else torch.cat(self.deq)
        mod = torch.tensor(self.rows, dtype=torch.int64)
        return store, mod, torch.cumsum(mod, 0) - mod

    def boundaries(self, t: int):
        """Row 0, the last row and the rows on both sides of every range start of table t."""
        n = self.rows[t]
        b = {0, n - 1}
        for lo, _, _ in self.ranges[t][1:]:
            b |= {lo - 1, lo}
        return sorted(v for v in b if 0 <= v < n)

    def owner_of(self, t: int, v: int) -> int:
        return next(r for r, (lo, n, _) in enumerate(self.ranges[t]) if lo <= v < lo + n)

    def ids(self, B: int, col0: int, hot: int, gen: torch.Generator, hot_ids: int = 64) -> torch.Tensor:
        """int64 [B, col0 + T * hot]: the skewed stream (x 67) with every boundary row
        of every table planted (candidate i takes table t's i-th boundary),
        half of the planted ids negative, the others with a multiple of the
        table's rows added (both fit int32)."""
        # the stream's hot ids 0 .. hot_ids - 1 become rows 0, 67, .. of the 4099: every rank's
        # range holds some of them, so from every rank there are hot REMOTE rows to cache
        ids = pc.skewed(B, col0 + self.T * hot, gen, hot_ids=hot_ids) * 67
        for t in range(self.T):
            for i, v in enumerate(self.boundaries(t)):
                if i < B:
                    ids[i, col0 + t * hot + i % hot] = v - 7 * self.rows[t] if i % 2 == 0 else v + 1000 * self.rows[t]
        return ids

    def spread_bag(self, t: int = 0):
        """Three rows of table t living on three different ranks (None when the table is not spread over all)."""
        rr = self.ranges[t]
        if any(n == 0 for _, n, _ in rr):
            return None
        return [lo for lo, _, _ in rr]


def bad_ranges(rs: RowStores):
    """(what, ranges) - each malformed in one way: a gap, a decreasing start,
    a total that is not the table's rows, a range past its store."""
    def edit(t, r, seg):
        out = [list(rr) for rr in rs.ranges]
        out[t][r] = seg
        return out

    t = next(t for t in range(rs.T) if t not in rs.whole and rs.rows[t] == ROWS)
    (lo0, n0, o0), (lo1, n1, o1), (lo2, n2, o2) = rs.ranges[t]
    store2 = rs.row_codes[2].shape[0]
    return [("gap", edit(t, 1, (lo1 + 1, n1 - 1, o1))),
            ("decreasing", edit(t, 2, (lo1 - 1, n2, o2))),
            ("total", edit(t, 2, (lo2, n2 - 1, o2))),
            ("store", edit(t, 2, (lo2, n2, store2 - n2 + 1)))]
