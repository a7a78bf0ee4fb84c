"""Shared cases of the fp8 peer-lookup tests (tests/test_peer_fp8_cpu.py,
tests/test_peer_fp8_gpu.py): two stores of e4m3 codes standing in for two
ranks, their bf16 twins on the dequantised rows, and the rounding-free probe
of the fused kernel with its fp32 and float64 references."""
import torch

from distributed_tf_serving_amd import ops
from distributed_tf_serving_amd.parallel.hot_cache import PeerTables

F8 = torch.float8_e4m3fn
# code bytes: +-448, +-the smallest subnormal, +-0, the smallest normal, 1.0
EXTREMES = torch.tensor([0x7E, 0xFE, 0x01, 0x81, 0x00, 0x80, 0x08, 0x38], dtype=torch.uint8)


def random_codes(n: int, gen: torch.Generator) -> torch.Tensor:
    """[n, 64] e4m3 codes, every finite byte (0x7F / 0xFF, the NaNs, left out)."""
    b = torch.randint(0, 0x7F, (n, 64), generator=gen, dtype=torch.uint8)
    sign = torch.randint(0, 2, (n, 64), generator=gen, dtype=torch.uint8) << 7
    return (b | sign).view(F8)


def table_scales(T: int) -> torch.Tensor:
    return (2.0 ** -(torch.arange(T) % 5).float())


def remote_half(T: int):
    """About half the tables on the other rank (odd tables; table 0 when T = 1)."""
    return tuple(range(1, T, 2)) if T > 1 else (0,)


class TwoStores:
    """Rank 0's view of tables laid out [T x rows] in each of two stores
    (table t's rows live in store owner[t]): the fp8 stores + scales, and the
    bf16 stores holding exactly the dequantised values."""

    def __init__(self, T, rows, remote, gen, scale=None, codes=None):
        self.T, self.rows, self.remote = T, rows, tuple(remote)
        self.scale = table_scales(T) if scale is None else scale
        self.codes = codes if codes is not None else [random_codes(T * rows, gen) for _ in range(2)]
        per_row = self.scale.repeat_interleave(rows).view(-1, 1)
        self.deq = []
        for c in self.codes:
            v = c.float() * per_row
            assert torch.equal(v.to(torch.bfloat16).float(), v)  # code x power of two is a bf16 value
            self.deq.append(v.to(torch.bfloat16))
        self.owner = [1 if t in self.remote else 0 for t in range(T)]
        self.off = [t * rows for t in range(T)]

    def plant(self, table: int, row: int, code_bytes: torch.Tensor) -> None:
        """Code bytes into row `row` of `table` where the table lives (and its dequantised twin)."""
        s, g = self.owner[table], self.off[table] + row
        self.codes[s].view(torch.uint8)[g] = code_bytes
        self.deq[s][g] = (self.codes[s][g].float() * self.scale[table]).to(torch.bfloat16)

    def _split(self, stores, chunk_shift, dev):
        stores = [s.to(dev) for s in stores]
        if chunk_shift is not None:  # chunks = views of the store; the kernels only see chunk addresses
            stores = [list(torch.split(s, 1 << chunk_shift)) for s in stores]
        return stores

    def peer_fp8(self, chunk_shift=None, dev="cpu") -> PeerTables:
        return PeerTables(self._split(self.codes, chunk_shift, dev), self.owner, self.off, [self.rows] * self.T,
                          rank=0, chunk_shift=chunk_shift, scale=self.scale)

    def peer_bf16(self, chunk_shift=None, dev="cpu") -> PeerTables:
        return PeerTables(self._split(self.deq, chunk_shift, dev), self.owner, self.off, [self.rows] * self.T,
                          rank=0, chunk_shift=chunk_shift)

    def local(self):
        """The concatenated code store every table's rows are in, for
        ops.dot_interaction_gather_fp8: (codes [T x rows, 64], modulo_f, offset_f)."""
        q = torch.cat([self.codes[self.owner[t]].view(torch.uint8)[t * self.rows:(t + 1) * self.rows]
                       for t in range(self.T)]).view(F8)
        return q, torch.full((self.T,), self.rows, dtype=torch.int64), torch.arange(self.T, dtype=torch.int64) * self.rows


def skewed(B, F, gen, hot_ids=40):
    """ids mostly drawn from a few hot values (the cache has something to hold), some negative."""
    ids = torch.randint(-(1 << 40), 1 << 40, (B, F), generator=gen)
    hot = torch.randint(0, hot_ids, (B, F), generator=gen)
    pick = torch.rand(B, F, generator=gen) < 0.8
    return torch.where(pick, hot, ids)


# ---------------------------------------------------------------- exact probe
def exact_probe(T: int, B: int = 37, rows: int = 200):
    """Rounding-free inputs of the fused kernel: integer codes and dense in
    [-2, 2], scales 1 and 2^-3 alternating per table, half the tables remote.
    Every product is a multiple of 2^-6 below 4 in magnitude and every dot is
    a sum of 64 of them, so below 256: fp32 accumulation rounds nothing in
    any order. Returns (TwoStores, dense bf16 [B, 64], ids int64 [B, T])."""
    g = torch.Generator().manual_seed(1000 + T)
    codes = [torch.randint(-2, 3, (T * rows, 64), generator=g).float().to(F8) for _ in range(2)]
    scale = torch.where(torch.arange(T) % 2 == 0, 1.0, 0.125).float()
    ts = TwoStores(T, rows, remote_half(T), g, scale=scale, codes=codes)
    dense = torch.randint(-2, 3, (B, 64), generator=g).to(torch.bfloat16)
    ids = torch.randint(-(1 << 40), 1 << 40, (B, T), generator=g)
    return ts, dense, ids


def probe_reference(ts: TwoStores, dense: torch.Tensor, ids: torch.Tensor, dtype):
    """[dense | lower triangle of V V^T | zero pad] in `dtype` arithmetic, V =
    (dense, row of table 0, ..): the interaction's contract, written out."""
    B, T = ids.shape
    v = torch.remainder(ids, ts.rows)
    rows = torch.stack([ts.codes[ts.owner[t]][ts.off[t] + v[:, t]].to(dtype) * ts.scale[t].to(dtype)
                        for t in range(T)], 1)                     # [B, T, 64]
    V = torch.cat([dense.to(dtype).unsqueeze(1), rows], 1)          # [B, T + 1, 64]
    G = torch.einsum("bik,bjk->bij", V, V)
    i, j = torch.tril_indices(T + 1, T + 1, offset=-1)
    used = 64 + (T + 1) * T // 2
    out = torch.zeros(B, ops.interaction_cols(T, 64), dtype=dtype)
    out[:, :64] = dense.to(dtype)
    out[:, 64:used] = G[:, i, j]
    return out
