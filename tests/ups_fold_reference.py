"""TEST-ONLY (no tests here): float64 restatements of the upsample conv, shared by tests/test_ups_fold_cpu.py and
tests/test_gpu_ups_fold.py.  Activations NHWC, weights packed as ``engine.pack_conv`` / ``engine.fold_ups_weight`` leave
them."""
import torch
import torch.nn.functional as Fn


def phase_conv(x, w4):
    """x [B,Hi,Wi,C], w4 [4][N][4C] -> [B,2Hi,2Wi,N]: phase 2 py + px reads the 2x2 window with origin
    (y + py - 1, x + px - 1), zero outside the image, taps in (dy, dx) order, and is stored at (2y + py, 2x + px)."""
    b, hi, wi, c = x.shape
    n = w4.shape[1]
    out = torch.zeros(b, 2 * hi, 2 * wi, n, dtype=x.dtype)
    xp = Fn.pad(x, (0, 0, 1, 1, 1, 1))                      # one zero pixel all round
    for py in range(2):
        for px in range(2):
            w = w4[2 * py + px].reshape(n, 2, 2, c)
            acc = torch.zeros(b, hi, wi, n, dtype=x.dtype)
            for dy in range(2):
                for dx in range(2):
                    win = xp[:, py + dy:py + dy + hi, px + dx:px + dx + wi]      # input pixel (y + py - 1 + dy, x + px - 1 + dx)
                    acc += win @ w[:, dy, dx].T
            out[:, py::2, px::2] = acc
    return out


def unfolded(x, w9):
    """conv3x3(nearest2x(x), pad 1) -> [B,2Hi,2Wi,N]; w9 [N][9C], K = (tap, cin)."""
    n, c = w9.shape[0], x.shape[-1]
    up = x.permute(0, 3, 1, 2).repeat_interleave(2, 2).repeat_interleave(2, 3)
    return Fn.conv2d(up, w9.reshape(n, 3, 3, c).permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
