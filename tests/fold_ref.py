"""Float64 references of the encoder's kernels, one function per kernel (stage) -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_fold_reference.py (CPU: the staged references chained reproduce oracle.bert_oracle.forward) and
tests/test_fold_kernels_gpu.py (GPU: every kernel against its stage).  Every function is written the plain way -- a LayerNorm is
mean / variance / normalise, never the folded algebra rs (A W'^T - mu c1) + c2 the kernels use -- and rounds nothing: callers hand in
inputs that are already bf16-representable where the kernel reads bf16.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24  # unit roundoff of f32


def bf16_round(a):
    """f32 -> nearest-even bf16, returned as f32 (what f32_to_bf16_kernel and the epilogues do)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def bf16_ulp(ref):
    """Spacing of bf16 numbers at |ref| (8 significant bits)."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126))) - 7)


def gelu(x):
    from scipy.special import erf

    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


# ---- layouts ---------------------------------------------------------------------------------------------------------
def block64(a):
    """[M, N] -> [N / 64, M, 64] (SC_LDC_BLOCKED64: 64-column blocks, each contiguous over the rows)."""
    M, N = a.shape
    return np.ascontiguousarray(a.reshape(M, N // 64, 64).transpose(1, 0, 2))


def unblock64(a, M, N):
    return np.ascontiguousarray(np.asarray(a).reshape(N // 64, M, 64).transpose(1, 0, 2).reshape(M, N))


def slot_stats(x, width=256):
    """Partial row statistics as the producing epilogues leave them: [cols / width][M][2] = (sum, sum of squares) per slot, float64."""
    x = np.asarray(x, np.float64)
    M, K = x.shape
    t = x.reshape(M, K // width, width)
    return np.ascontiguousarray(np.stack([t.sum(-1), (t * t).sum(-1)], axis=-1).transpose(1, 0, 2))


def embed_slot_stats(x, slots):
    """embed_raw_kernel's layout: slot 0 carries the sums of the whole row, the other slots are zero."""
    x = np.asarray(x, np.float64)
    out = np.zeros((slots, x.shape[0], 2))
    out[0, :, 0], out[0, :, 1] = x.sum(1), (x * x).sum(1)
    return out


def finalise(stats, K, eps):
    """(mu, rs) [M, 2] from partial statistics [slots][M][2], in float64."""
    s = np.asarray(stats, np.float64).sum(0)
    mu = s[:, 0] / K
    var = np.maximum(s[:, 1] / K - mu * mu, 0.0)
    return np.stack([mu, 1.0 / np.sqrt(var + eps)], axis=1)


# ---- stages ----------------------------------------------------------------------------------------------------------
def row_moments(x):
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return mu, var


def normalise(x, eps):
    """(x - mean) / sqrt(var + eps) per row: a LayerNorm without gamma / beta."""
    mu, var = row_moments(x)
    return (np.asarray(x, np.float64) - mu) / np.sqrt(var + eps)


def layernorm(x, g, b, eps):
    return normalise(x, eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def embed_sum(ids, wemb, pemb, temb, max_pos, dtype=np.float64):
    """(word + position) + type per token of ids [B, S]: ids clamp to [0, vocab), positions to max_pos - 1; [B*S, H] in `dtype`."""
    ids = np.asarray(ids)
    B, S = ids.shape
    w = np.asarray(wemb, dtype)[np.clip(ids.reshape(-1), 0, wemb.shape[0] - 1)]
    if pemb is not None:
        w = w + np.asarray(pemb, dtype)[np.minimum(np.tile(np.arange(S), B), max_pos - 1)]
    return w + np.asarray(temb, dtype).reshape(-1, w.shape[1])[0]


def lna_plain(A, W, gamma, beta, bias, eps, act=None):
    """LayerNorm(A; gamma, beta) W^T + bias (+ GELU): what an EPI_LNA_* GEMM stands for."""
    y = layernorm(A, gamma, beta, eps) @ np.asarray(W, np.float64).T + np.asarray(bias, np.float64)
    return gelu(y) if act == "gelu" else y


def lna_with_folded_weight(A, Wf, c2, eps, act=None):
    """The same with the weight already multiplied by gamma (W' = W diag(gamma)) and c2 = bias + W beta: normalise, multiply, add."""
    y = normalise(A, eps) @ np.asarray(Wf, np.float64).T + np.asarray(c2, np.float64)
    return gelu(y) if act == "gelu" else y


def rope_rotate(y, S, theta, ncols):
    """Rotate-half rotary embedding of the first ncols columns (heads of 64) of y [M, N]; row r has position r & (S - 1)."""
    y = np.array(y, np.float64)
    M = y.shape[0]
    pos = (np.arange(M) & (S - 1)).astype(np.float64)
    ang = pos[:, None] * (float(theta) ** (-2.0 * np.arange(32) / 64.0))[None, :]
    c, s = np.cos(ang), np.sin(ang)
    for h0 in range(0, ncols, 64):
        lo, hi = y[:, h0:h0 + 32].copy(), y[:, h0 + 32:h0 + 64].copy()
        y[:, h0:h0 + 32] = lo * c - hi * s
        y[:, h0 + 32:h0 + 64] = hi * c + lo * s
    return y


def resln(A, W, bias_plus_beta, gam, R, eps):
    """A W^T + (b + beta) + normalise(R) gam = A W^T + b + LayerNorm(R; gam, beta): what EPI_RESLN_STATS stands for."""
    return (np.asarray(A, np.float64) @ np.asarray(W, np.float64).T + np.asarray(bias_plus_beta, np.float64)
            + normalise(R, eps) * np.asarray(gam, np.float64))


def attention(qkv, lens, B, S, heads, slopes=None):
    """qkv [B*S, 3H] rows = [Q | K | V] -> softmax(Q K^T / 8 + key mask - slope_h |i - j|) V, [B*S, H]; one (chunk, head) at a time."""
    H = heads * 64
    x = np.asarray(qkv, np.float64).reshape(B, S, 3, heads, 64)
    lens = np.clip(np.asarray(lens), 1, S)
    out = np.empty((B, S, heads, 64))
    dist = np.abs(np.arange(S)[:, None] - np.arange(S)[None, :]).astype(np.float64)
    for b in range(B):
        n = int(lens[b])
        for h in range(heads):
            s = x[b, :, 0, h] @ x[b, :n, 1, h].T / 8.0
            if slopes is not None:
                s = s - float(slopes[h]) * dist[:, :n]
            p = np.exp(s - s.max(-1, keepdims=True))
            out[b, :, h] = (p / p.sum(-1, keepdims=True)) @ x[b, :n, 2, h]
    return out.reshape(B * S, H)


def mean_pool(x, lens, S, normalize=False):
    x = np.asarray(x, np.float64)
    lens = np.clip(np.asarray(lens), 1, S)
    B = lens.size
    xb = x[: B * S].reshape(B, S, -1)
    out = np.stack([xb[b, : lens[b]].mean(0) for b in range(B)])
    if normalize:
        out = out / np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-12)
    return out


def mean_pool_ln(y, gamma, beta, eps, lens, S):
    return mean_pool(layernorm(y, gamma, beta, eps), lens, S)


def geglu(h):
    h = np.asarray(h, np.float64)
    F = h.shape[1] // 2
    return gelu(h[:, :F]) * h[:, F:]


# ---- test data -------------------------------------------------------------------------------------------------------
ORDINARY, LARGE_MEAN, TINY_VAR, ZERO, UNEVEN = range(5)


def make_rows(rng, M, K):
    """bf16-representable rows [M, K] of five populations in one matrix, and the population of every row:
    ORDINARY zero-mean N(0,1); LARGE_MEAN N(0,1) + mu with |mu| / sigma in [1, 8]; TINY_VAR 3 + 2^-6 {-2..2} (non-zero rows of
    near-zero variance, |mu| / sigma ~ 140); ZERO all-zero rows (the padding rows; the last 37 rows too); UNEVEN rows whose energy
    sits in one 256-column slot (8 N(0,1) there, 0.05 N(0,1) elsewhere), so that the partial statistics differ by 4 orders of
    magnitude between the slots."""
    kind = np.array([ORDINARY] * 9 + [LARGE_MEAN] * 3 + [TINY_VAR, ZERO, UNEVEN, UNEVEN])[np.arange(M) % 16]
    kind[M - 37:] = ZERO
    A = rng.standard_normal((M, K))
    lm = kind == LARGE_MEAN
    A[lm] += (rng.uniform(1.0, 8.0, lm.sum()) * rng.choice([-1.0, 1.0], lm.sum()))[:, None]
    tv = kind == TINY_VAR
    A[tv] = 3.0 + 2.0 ** -6 * rng.integers(-2, 3, (int(tv.sum()), K))
    A[kind == ZERO] = 0.0
    for r in np.nonzero(kind == UNEVEN)[0]:
        j = int(rng.integers(0, K // 256))
        A[r] *= 0.05
        A[r, 256 * j:256 * j + 256] *= 160.0
    return bf16_round(A.astype(np.float32)), kind
