"""What the per-op GPU tests share (test_ops_gpu, test_attn_bf_gpu, test_row_ops_gpu, test_gemm_gpu, test_block_rows_gpu): device arrays, a fresh state
block, the relative error, sentinel-filled buffers and the fp64 attention core."""
import numpy as np
import torch

SENTINEL = 0x7FC0BEEF          # a quiet NaN with a payload


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).cuda().contiguous()


def relerr(got, want):
    want = np.asarray(want, np.float64)
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))


class Pad:
    """[rows, ld] floats on the device plus a tail, all SENTINEL; regions = [(first column, columns)] are what a kernel may touch,
    optionally filled with data (one array per region).  lead: SENTINEL words in front of the matrix (t is the matrix: with lead = 1
    it starts one float past the allocation's boundary)."""

    def __init__(self, rows, ld, regions, data=None, tail=9, lead=0):
        self.rows, self.ld, self.regions = rows, ld, regions
        host = np.full(lead + rows * ld + tail, SENTINEL, np.uint32).view(np.float32)
        self.inside = np.zeros(rows * ld + tail, bool)
        body, inside = host[lead:lead + rows * ld].reshape(rows, ld), self.inside[:rows * ld].reshape(rows, ld)
        for k, (off, cols) in enumerate(regions):
            assert off + cols <= ld
            inside[:, off:off + cols] = True
            if data is not None:
                body[:, off:off + cols] = np.asarray(data if len(regions) == 1 else data[k], np.float32).reshape(rows, cols)
        self.whole = torch.from_numpy(host.copy()).cuda()
        self.t, self.lead = self.whole[lead:], lead

    def read(self, k=0):
        off, cols = self.regions[k]
        return self.t[:self.rows * self.ld].reshape(self.rows, self.ld)[:, off:off + cols].contiguous().cpu().numpy()

    def untouched(self):
        bits = self.whole.cpu().numpy().view(np.uint32)
        return bool((bits[:self.lead] == SENTINEL).all() and (bits[self.lead:][~self.inside] == SENTINEL).all())


def new_state(step=0):
    st = torch.zeros(16, dtype=torch.float32, device="cuda")          # CR_STATE_FLOATS
    st[4:5].view(torch.int32)[0] = step
    return st


def attn_core_ref(Q, K, V, kvalid, qvalid, resid, H, keep=None, rate=0.0, mm=None, softmax=None):
    """modules.py:208-269 from the projected Q/K/V on (float64 torch).  mm(a, b, site) / softmax(scores): stand-ins for the two matrix
    products ("scores", "pv") and the softmax (the rounding model of plain bf16: test_attn_bf_gpu.rounded_model); default: exact."""
    N, T, C = Q.shape
    d = C // H
    mm = mm or (lambda a, b, site: a @ b)
    softmax = softmax or (lambda s: torch.softmax(s, -1))
    Q_ = torch.cat(torch.split(Q, d, dim=2), 0); K_ = torch.cat(torch.split(K, d, dim=2), 0); V_ = torch.cat(torch.split(V, d, dim=2), 0)
    out = mm(Q_, K_.transpose(1, 2), "scores") / d ** 0.5
    km = kvalid.repeat(H, 1)[:, None, :].expand(-1, T, -1)
    pad = torch.full_like(out, float(-2 ** 32 + 1))
    out = torch.where(km == 0, pad, out)
    tril = torch.tril(torch.ones(T, T, dtype=out.dtype))
    out = torch.where(tril[None] == 0, pad, out)
    out = softmax(out)
    out = out * qvalid.repeat(H, 1)[:, :, None]
    if keep is not None:
        out = out * torch.tensor(keep, dtype=out.dtype) / (1.0 - rate)
    w = out
    out = mm(out, V_, "pv")
    out = torch.cat(torch.split(out, N, dim=0), 2)
    return out + resid, w
