"""Sampled-pixel reference of the contextual attention (oracle/sketchedit_oracle.py contextual_attention, editline_g.py:203-207).

The oracle forms the whole L x L score matrix, which at 1080p (L = 32 026 keys) or 2048x2048 (65 025) is far too large for a
test.  This restates the same arithmetic for a chosen set of output pixels only:
  1. keys: unfold(xn) over all L keys (xn = x / ||x|| per image and channel; rounded to `dt` as the oracle's _r does);
  2. the score rows of only the <= 4 queries whose 4x4 patches (stride 2) cover a chosen pixel, the multiplicative key
     validity (> 0.1 hole-free, an invalid key keeps logit 0) and the softmax over all keys (P rounded to `dt`);
  3. the overlap-add of P . V at those pixels (no normalisation; the result rounded to `dt`).
Cost O(n_queries * L * 1536).  Pixels in aligned 2x2 groups share their four queries.  Products and sums run in float64
(fp32 mode, dt=None): the reference is then closer to exact than the oracle's own fp32 einsum.
"""
import numpy as np
import torch
import torch.nn.functional as F


def _r(t, dt):
    return t if dt is None else t.to(dt).to(torch.float32)


def sample_pixels(B, h, w, n, seed=0):
    """-> int array (m, 3) of (image, y, x), m >= n: aligned 2x2 groups at random positions plus every corner, the middle of
    every border and of the last class-grid row / column (y, x = h - 2, w - 2 and their neighbours)."""
    rng = np.random.default_rng(seed)
    groups = set()
    for b in range(B):
        for gy in (0, h // 4, h // 2 - 1):
            for gx in (0, w // 4, w // 2 - 1):
                groups.add((b, gy, gx))
        for g in range(1, h // 2 - 1, max(1, (h // 2) // 8)):
            groups.add((b, g, 0)); groups.add((b, g, w // 2 - 1))
        for g in range(1, w // 2 - 1, max(1, (w // 2) // 8)):
            groups.add((b, 0, g)); groups.add((b, h // 2 - 1, g))
    while len(groups) * 4 < n:
        groups.add((int(rng.integers(B)), int(rng.integers(h // 2)), int(rng.integers(w // 2))))
    pix = [(b, 2 * gy + dy, 2 * gx + dx) for (b, gy, gx) in sorted(groups) for dy in (0, 1) for dx in (0, 1)]
    return np.array(pix, dtype=np.int64)


def colreduce_rn_fp32(x, splits=128):
    """1 / sqrt(sum_hw x^2 + 1e-8) per (image, channel) in the summation order of the library's deterministic column
    reduction (se_misc.hip colreduce_partial_kernel / _final_kernel, fp32, 24 channel granules of 4 -> 10 pixel groups per
    split): fmaf chains over every 10th pixel of a split, the 10 groups in order, the splits in order.  -> (B, 96) float32."""
    x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, np.float32)
    B, C, h, w = x.shape
    HW = h * w
    v = x.reshape(B, C, HW).astype(np.float64)
    per = (HW + splits - 1) // splits
    groups = 256 // (C // 4)
    rn = np.empty((B, C), np.float32)
    for b in range(B):
        parts = []
        for sp in range(splits):
            p0, p1 = sp * per, min(HW, sp * per + per)
            accs = []
            for g in range(groups):
                a = np.zeros(C, np.float32)
                for pp in range(p0 + g, p1, groups):
                    a = (v[b, :, pp] * v[b, :, pp] + a.astype(np.float64)).astype(np.float32)      # fmaf: one rounding
                accs.append(a)
            r = accs[0]
            for a in accs[1:]:
                r = (r + a).astype(np.float32)
            parts.append(r)
        r = np.zeros(C, np.float32)
        for a in parts:
            r = (r + a).astype(np.float32)
        rn[b] = (np.float32(1.0) / np.sqrt(r + np.float32(1e-8))).astype(np.float32)
    return torch.from_numpy(rn)


def sampled_attention(x, mask_full, pix, dt=None, scale=10.0, th=0.1, rn=None):
    """x (B, 96, h, w) and mask_full (B, 1, 4h, 4w) as float32 arrays or CPU tensors; pix (n, 3) of (image, y, x).
    -> (n, 96) float32 tensor: the oracle's attention output at those pixels.  `rn` (B, 96), optional: the key norm
    1 / ||x|| to use instead of the oracle's own fp32 reduction (e.g. colreduce_rn_fp32)."""
    x = torch.as_tensor(np.asarray(x, np.float32) if not torch.is_tensor(x) else x).float()
    mask_full = torch.as_tensor(np.asarray(mask_full, np.float32) if not torch.is_tensor(mask_full) else mask_full).float()
    B, C, h, w = x.shape
    hs, ws = (h - 4) // 2 + 1, (w - 4) // 2 + 1
    pix = np.asarray(pix, np.int64)
    out = torch.zeros(len(pix), C)
    with torch.no_grad():
        if rn is None:
            xn = _r(x / torch.sqrt((x * x).sum(3, keepdim=True).sum(2, keepdim=True) + 1e-8), dt)
        else:
            xn = _r(x * torch.as_tensor(rn).float().view(B, C, 1, 1), dt)
        valid = 1.0 - F.avg_pool2d(mask_full, 4, 4)
        mm = F.unfold(valid, 4, stride=2).view(B, 4, 4, -1).mean(2).mean(1)      # (B, L), as the oracle averages it
        for b in np.unique(pix[:, 0]):
            sel = np.nonzero(pix[:, 0] == b)[0]
            K = F.unfold(xn[b:b + 1], 4, stride=2)[0]                           # (1536, L)
            kv = (mm[b] > th).float()                                           # (L,)
            # the queries covering each chosen pixel: patch (iy, ix) with 2 iy <= y <= 2 iy + 3
            cover = []
            qset = {}
            for n in sel:
                y, xx = int(pix[n, 1]), int(pix[n, 2])
                for iy in range(max(0, (y - 2) // 2), min(hs - 1, y // 2) + 1):
                    for ix in range(max(0, (xx - 2) // 2), min(ws - 1, xx // 2) + 1):
                        if 0 <= y - 2 * iy < 4 and 0 <= xx - 2 * ix < 4:
                            cover.append((n, qset.setdefault((iy, ix), len(qset)), y - 2 * iy, xx - 2 * ix))
            qs = sorted(qset, key=qset.get)
            Q = torch.stack([x[b, :, 2 * iy:2 * iy + 4, 2 * ix:2 * ix + 4].reshape(-1) for iy, ix in qs])      # (nq, 1536)
            if dt is None:
                Q, K, kv = Q.double(), K.double(), kv.double()
            S = (Q @ K) * kv[None, :]                                           # (nq, L)
            P = _r(torch.softmax(S * scale, dim=1).float(), dt).to(S.dtype)
            # values: raw patches; V[c, ky, kx, j] = x[2 jy + ky, 2 jx + kx, c]
            V = F.unfold(x[b:b + 1], 4, stride=2)[0].view(C, 4, 4, -1).to(S.dtype)
            acc = torch.zeros(len(pix), C, dtype=S.dtype)
            for n, qi, ky, kx in cover:
                acc[n] += V[:, ky, kx, :] @ P[qi]
            out[sel] = acc[sel].float()
            del K, V
    return _r(out, dt)


def gather_pixels(full, pix):
    """full (B, 96, h, w) array / tensor -> (n, 96) tensor at pix."""
    t = full.detach().cpu() if torch.is_tensor(full) else torch.from_numpy(np.asarray(full, np.float32))
    p = torch.from_numpy(np.asarray(pix, np.int64))
    return t[p[:, 0], :, p[:, 1], p[:, 2]]


def contextual_attention_chunked(x, mask_full, dt=None, rows=8, scale=10.0, th=0.1):
    """The oracle's contextual_attention (same signature and result: (out, None) -- no `similar`) computed in chunks of
    `rows` output class rows, so that memory stays O(rows * R) instead of L^2.  Space-to-depth restatement of the same
    arithmetic: E = X XN^T over 384-vectors, S = the 2x2 box sum of E on the query / key sub-grid, key
    validity as a multiplicative zero, softmax over all keys, out[2r+cls] = sum_s P~[r][s] x[2s+cls] with P~[r][s] =
    sum_d P[r-d][s-d].  fp32 like the oracle (only the summation order differs); `dt` rounds xn, P and the output where the
    oracle does."""
    x = torch.as_tensor(x).float()
    mask_full = torch.as_tensor(mask_full).float()
    B, C, h, w = x.shape
    hc, wc = h // 2, w // 2
    hs, ws = hc - 1, wc - 1
    R = hc * wc
    out = torch.empty_like(x)
    with torch.no_grad():
        xn = _r(x / torch.sqrt((x * x).sum(3, keepdim=True).sum(2, keepdim=True) + 1e-8), dt)
        valid = 1.0 - F.avg_pool2d(mask_full, 4, 4)
        mm = F.unfold(valid, 4, stride=2).view(B, 4, 4, -1).mean(2).mean(1)
        for b in range(B):
            # X[r][(py, px, c)] = x[c, 2 ry + py, 2 rx + px]
            X = x[b].view(C, hc, 2, wc, 2).permute(1, 3, 2, 4, 0).reshape(R, 4 * C).contiguous()
            XN = xn[b].view(C, hc, 2, wc, 2).permute(1, 3, 2, 4, 0).reshape(R, 4 * C).contiguous()
            kv = (mm[b] > th).float().view(1, 1, hs, ws)
            ob = torch.empty(hc, wc, 4 * C)
            for r0 in range(0, hc, rows):
                r1 = min(hc, r0 + rows)
                q0, q1 = max(0, r0 - 1), min(hs, r1)              # queries r - d of the output rows [r0, r1)
                e0, e1 = q0, q1 + 1                                 # E rows q + d
                E = (X[e0 * wc:e1 * wc] @ XN.t()).view(e1 - e0, wc, hc, wc)
                nq = q1 - q0
                S = (E[:nq, :ws, :hs, :ws] + E[:nq, 1:, :hs, 1:]) + E[1:nq + 1, :ws, 1:, :ws] + E[1:nq + 1, 1:, 1:, 1:]
                del E
                S = S * kv
                P = _r(torch.softmax((S * scale).reshape(nq, ws, hs * ws), dim=2), dt).view(nq, ws, hs, ws)
                del S
                Pt = torch.zeros(r1 - r0, wc, hc, wc)
                for dy in (0, 1):
                    for dx in (0, 1):
                        # P~[ry, rx, sy, sx] += P[ry - dy, rx - dx, sy - dy, sx - dx] for queries inside [q0, q1)
                        ya, yb = max(r0, q0 + dy), min(r1, q1 + dy)
                        if ya >= yb:
                            continue
                        Pt[ya - r0:yb - r0, dx:dx + ws, dy:dy + hs, dx:dx + ws] += P[ya - dy - q0:yb - dy - q0]
                del P
                ob[r0:r1] = (Pt.view((r1 - r0) * wc, R) @ X).view(r1 - r0, wc, 4 * C)
                del Pt
            out[b] = ob.view(hc, wc, 2, 2, C).permute(4, 0, 2, 1, 3).reshape(C, h, w)
    return _r(out, dt), None
