import ctypes as C

import numpy as np


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def row_rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b, axis=-1) / (np.linalg.norm(b, axis=-1) + 1e-30)


def to16(x_np, dtype, device):
    """numpy fp32 -> CUDA 16-bit tensor of the given operand type ('fp16' | 'bf16')."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x_np, dtype=np.float32)).to(device)
    return t.to(torch.float16 if dtype == "fp16" else torch.bfloat16).contiguous()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch_families(fn):
    """(kernel family, epilogue, N, K) -> launches that the call ``fn()`` issues (leaf_prof_begin / leaf_prof_end_shapes; family ids:
    leaf_amd/csrc/kernels.h leaf_gemm_family, 8 = the fused QKV + attention launch)"""
    from leaf_amd import _lib
    lib = _lib.lib()
    lib.leaf_prof_begin()
    fn()
    ng = 64
    ms, fl, by = (C.c_double * ng)(), (C.c_double * ng)(), (C.c_double * ng)()
    rows, info, n = (C.c_int64 * ng)(), (C.c_int32 * (4 * ng))(), C.c_int(0)
    _lib.check(lib.leaf_prof_end_shapes(ms, fl, by, rows, info, ng, C.byref(n)), "prof")
    out = {}
    for i in range(n.value):
        key = ((info[4 * i] % 1024) // 32, info[4 * i] % 16, info[4 * i + 1], info[4 * i + 2])
        out[key] = out.get(key, 0) + info[4 * i + 3]
    return out


# north_star's embedding gate: rel-L2 <= 1e-3 PER ROW against the fp32 reference / oracle on the BASELINE.json towers (ViT-L, ViT-H, bigG).
# Round 4: tightened from 1.25e-3 after measuring every row these tests look at (tests/row_error_survey.py,
# profiles/r04_row_error_survey.txt: maxima 9.3e-4 ... 9.9e-4); the forward is deterministic, so a test that passes, passes again.
TOL_ROW = 1.0e-3


def trained_like_weights(cfg, seed=0, alpha=0.7, gain_sigma=0.5):
    """A text tower whose weights LOOK like a trained CLIP's as far as that can be synthesised offline (pretrained
    weights need the network): every GEMM weight gets a power-law singular spectrum s_i ~ i^-alpha (random near-orthogonal factors,
    Frobenius norm of the random init kept, so activations keep their scale), LayerNorm gains are log-normal per channel with a few
    large outlier channels, LayerNorm / linear biases are non-zero, token embeddings have a heavy-tailed norm distribution.  Starts
    from ``oracle.init_weights(cfg, seed=1)`` (shapes, names)."""
    from oracle import text_oracle as O
    rng = np.random.default_rng(seed)
    w = {k: v.copy() for k, v in O.init_weights(cfg, seed=1).items()}
    for k, v in w.items():
        if v.ndim == 2 and k.endswith(("in_proj_weight", "out_proj.weight", "c_fc.weight", "c_proj.weight")) or k == "text_projection":
            n, m = v.shape
            r = min(n, m)
            a = rng.standard_normal((n, r)).astype(np.float32) / np.sqrt(n)
            b = rng.standard_normal((m, r)).astype(np.float32) / np.sqrt(m)
            s = (np.arange(1, r + 1, dtype=np.float32) ** -alpha)
            new = (a * s[None, :]) @ b.T
            w[k] = (new * (np.linalg.norm(v) / np.linalg.norm(new))).astype(np.float32)
        elif k.endswith(("ln_1.weight", "ln_2.weight")) or k == "ln_final.weight":
            g = np.exp(gain_sigma * rng.standard_normal(v.shape)).astype(np.float32)
            g[rng.choice(v.size, 4, replace=False)] *= 6.0            # outlier channels
            w[k] = g
        elif k.endswith(("ln_1.bias", "ln_2.bias")) or k == "ln_final.bias":
            w[k] = (0.1 * rng.standard_normal(v.shape)).astype(np.float32)
        elif k.endswith("bias"):
            w[k] = (0.02 * rng.standard_normal(v.shape)).astype(np.float32)
        elif k == "token_embedding.weight":
            scale = np.exp(0.4 * rng.standard_normal((v.shape[0], 1))).astype(np.float32)      # heavy-tailed token norms
            w[k] = (v * scale).astype(np.float32)
    return w


# ---------------------------------------------------------------- float64 reference of the attention kernels' row modes
# (leaf_amd/csrc/attention.hip, qkv_attn.hip; the operation: nn.MultiheadAttention in ResidualAttentionBlock).  Plain numpy, no code
# shared with leaf_amd/: tests/test_gpu_attention_modes.py holds the kernels to it, tests/test_attention_ref_cpu.py pins it.
def round16(x, dtype):
    """float -> the nearest value of the 16-bit operand type ('fp16' | 'bf16'), as float64"""
    from oracle import text_oracle as O
    return (O.round_fp16(x) if dtype == "fp16" else O.round_bf16(x)).astype(np.float64)


def attn_assemble(own, cache, lens, prefix=None, base_cu=None, group=1, group_off=0, edit=False):
    """The full [prefix + len, 3d] q|k|v rows of every sequence (the `rowptr` rule of attention.hip, restated).
    Sequence s computes lens[s] positions behind its first prefix[s] ones; s >= group_off belongs to caption (s - group_off) // group,
    whose rows start at cache[base_cu[caption]].  Row modes: positions < prefix[s] are the caption's cache rows, the others the
    sequence's own rows (own = the sequences' rows back to back).  Single-edit mode: own is a [n_seq, 3d] table with ONE row per
    sequence, its position prefix[s]; every other position is the caption's cache row, and a sequence in front of group_off is
    caption s itself, cache rows only."""
    seqs, r = [], 0
    for s, L in enumerate(lens):
        L = int(L)
        p = int(prefix[s]) if prefix is not None else 0
        if edit:
            cap = s if s < group_off else (s - group_off) // group
            full = np.array(cache[base_cu[cap]: base_cu[cap] + p + L], np.float64)
            if s >= group_off:
                full[p] = own[s]
        else:
            full = np.array(own[r: r + L], np.float64)
            if p:
                cap = (s - group_off) // group
                full = np.concatenate([np.asarray(cache[base_cu[cap]: base_cu[cap] + p], np.float64), full])
        assert full.shape[0] == p + L
        seqs.append(full)
        r += L
    return seqs


def attn_seq_ref(seq, heads, model=None):
    """softmax(q k^T / 8 + causal mask) v per head of one sequence's [T, 3d] q|k|v rows -> [T, d], float64.
    model = 'fp16' | 'bf16': the rounding model of the kernels -- P rounded to the operand type before P V, the output rounded to it."""
    seq = np.asarray(seq, np.float64)
    T, d = seq.shape[0], heads * 64
    q, k, v = (seq[:, i * d:(i + 1) * d].reshape(T, heads, 64).transpose(1, 0, 2) for i in range(3))
    s = q @ k.transpose(0, 2, 1) / 8.0 + np.triu(np.full((T, T), -np.inf), 1)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    if model:
        p = round16(p, model)
    o = (p @ v).transpose(1, 0, 2).reshape(T, d)
    return round16(o, model) if model else o


def attn_slice(outs, prefix=None, eot=None):
    """The rows a launch must write, in its output order: positions >= prefix[s] of every sequence, or its single eot[s] row."""
    rows = []
    for s, o in enumerate(outs):
        if eot is not None:
            rows.append(o[int(eot[s]): int(eot[s]) + 1])
        else:
            rows.append(o[(int(prefix[s]) if prefix is not None else 0):])
    return np.concatenate(rows)


def lnfold_rows_ref(x16, wp, s_vec, c_vec, mean, rstd, dtype):
    """The q|k|v rows of the LN-folded projection (leaf_hip.h, leaf_op_gemm_lnfold): round16(rstd[m] (x16[m] . Wp[n] - mean[m] s[n]) +
    c[n]) in float64"""
    f = lambda a: np.asarray(a, np.float64)
    acc = f(x16) @ f(wp).T
    return round16(f(rstd)[:, None] * (acc - f(mean)[:, None] * f(s_vec)[None, :]) + f(c_vec)[None, :], dtype)


# ---------------------------------------------------------------- float64 references of the training backward's kernels on packed rows
# (leaf_amd/csrc/attention_bwd.hip, train.hip).  Plain numpy, no code shared with leaf_amd/: tests/test_gpu_backward_rows.py and
# test_layernorm_bwd hold the kernels to them, tests/test_backward_ref_cpu.py pins them against torch autograd / np.add.at.
def attn_bwd_seq_ref(seq, do, heads, ft, gt, model=None):
    """Backward of softmax(q k^T / 8 + causal mask) v per head of ONE sequence: seq [T, 3d] q|k|v rows (values of the forward type
    ft), do [T, d] (values of the gradient type gt) -> [T, 3d] dq|dk|dv in float64.  P comes from the operands as given; when
    ft != gt, q, k, v are rounded once to gt before the gradient products (the kernel's documented conversion: it is part of the
    operation, not of the error).  model: the kernel's three roundings to gt on top -- P before P^T dO, dS before its two products,
    the output."""
    seq, do = np.asarray(seq, np.float64), np.asarray(do, np.float64)
    T, d = seq.shape[0], heads * 64
    q, k, v = (seq[:, i * d:(i + 1) * d].reshape(T, heads, 64).transpose(1, 0, 2) for i in range(3))
    g = do.reshape(T, heads, 64).transpose(1, 0, 2)
    s = q @ k.transpose(0, 2, 1) / 8.0 + np.triu(np.full((T, T), -np.inf), 1)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    if ft != gt:
        q, k, v = round16(q, gt), round16(k, gt), round16(v, gt)
    dp = g @ v.transpose(0, 2, 1)
    ds = p * (dp - (p * dp).sum(-1, keepdims=True)) / 8.0
    if model:
        p, ds = round16(p, gt), round16(ds, gt)
    dq, dk, dv = ds @ k, ds.transpose(0, 2, 1) @ q, p.transpose(0, 2, 1) @ g
    out = np.concatenate([a.transpose(1, 0, 2).reshape(T, d) for a in (dq, dk, dv)], axis=1)
    return round16(out, gt) if model else out


def ln_bwd_ref(dy, x, g, eps, dtype=np.float64):
    """LayerNorm backward of every row in the arithmetic of `dtype` -> (dx [rows, d], xhat [rows, d]); dg = (dy * xhat).sum(0) and
    db = dy.sum(0) are the caller's.  dtype = np.float32 is the error MODEL of the fp32 kernels (same formula, same inputs)."""
    dy, x, g = (np.asarray(a, dtype) for a in (dy, x, g))
    d = dtype(x.shape[-1])
    mu = x.sum(-1, keepdims=True, dtype=dtype) / d
    xc = x - mu
    rstd = dtype(1) / np.sqrt((xc * xc).sum(-1, keepdims=True, dtype=dtype) / d + dtype(eps))
    xhat = xc * rstd
    dxhat = dy * g
    m1 = dxhat.sum(-1, keepdims=True, dtype=dtype) / d
    m2 = (dxhat * xhat).sum(-1, keepdims=True, dtype=dtype) / d
    return rstd * (dxhat - m1 - xhat * m2), xhat


def pool_project_bwd_ref(dout, xe, g, b, eps, proj, dtype=np.float64):
    """The chain behind the loss head: pooled = LN_final(xe) (xe [n, d] = the pooled rows), feat = pooled @ proj [d, D].
    dout [n, D] -> dict(pooled, dproj [d, D], dpooled [n, d], dx [n, d] (un-scaled), dg [d], db [d]) plus, for the derived
    accumulation bounds, the sums of absolute terms abs_dproj, abs_dpooled, abs_dg, abs_db."""
    dout, xe, g, b, proj = (np.asarray(a, dtype) for a in (dout, xe, g, b, proj))
    dpooled = dout @ proj.T
    dx, xhat = ln_bwd_ref(dpooled, xe, g, eps, dtype)
    pooled = xhat * g + b
    r = dict(pooled=pooled, dproj=pooled.T @ dout, dpooled=dpooled, dx=dx, dg=(dpooled * xhat).sum(0), db=dpooled.sum(0))
    if dtype is np.float64:
        mu = xe.mean(-1, keepdims=True)
        rstd = 1.0 / np.sqrt(((xe - mu) ** 2).mean(-1, keepdims=True) + eps)
        r["abs_dpooled"] = np.abs(dout) @ np.abs(proj).T
        r["abs_dproj"] = np.abs(pooled).T @ np.abs(dout)
        r["abs_dg"] = (r["abs_dpooled"] * (np.abs(xe) + np.abs(mu)) * rstd).sum(0)
        r["abs_db"] = r["abs_dpooled"].sum(0)
    return r


def embed_bwd_ref(dx, tokens, lens, ctx, vocab):
    """The embedding scatter on packed rows: dx [sum(lens), d], tokens [n_seq, ctx]; slot (s, p) is KEPT iff p < lens[s], its row is
    sum(lens[:s]) + p and its id is clamped to 0 .. vocab - 1.  -> (dtok [vocab, d], dpos [ctx, d], abs_dtok, abs_dpos, count
    [vocab]): sums of the kept rows, sums of their absolute values, kept rows per id.  Dense rows: lens = [ctx] * n_seq."""
    dx = np.asarray(dx, np.float64)
    d = dx.shape[1]
    dtok, dpos = np.zeros((vocab, d)), np.zeros((ctx, d))
    atok, apos = np.zeros((vocab, d)), np.zeros((ctx, d))
    count = np.zeros(vocab, np.int64)
    row = 0
    for s, L in enumerate(lens):
        for p in range(int(L)):
            t = min(max(int(tokens[s][p]), 0), vocab - 1)
            dtok[t] += dx[row]
            atok[t] += np.abs(dx[row])
            dpos[p] += dx[row]
            apos[p] += np.abs(dx[row])
            count[t] += 1
            row += 1
    assert row == dx.shape[0]
    return dtok, dpos, atok, apos, count


def fare_ref(feat, anchor, scale, norms=None):
    """TextFARE head (utils_AT.py:319-321): loss = mean_b sum_j (anchor - feat)^2, dout = scale * d loss / d feat [B, D]; with norms
    [B] (--normalize_fare) feat = f / max(||f||, 1e-12) and dout is the gradient with respect to f, through F.normalize.
    -> (loss, dout, abs_loss, abs_dout): the last two are the sums of absolute terms behind loss and behind each dout element."""
    f, a = np.asarray(feat, np.float64), np.asarray(anchor, np.float64)
    B = f.shape[0]
    df = f - a
    loss = (df * df).sum(-1).mean()
    g = 2.0 / B * scale * df
    abs_g = np.abs(g)
    if norms is not None:
        inv = 1.0 / np.maximum(np.asarray(norms, np.float64), 1e-12)[:, None]
        dot = (f * g).sum(-1, keepdims=True)
        abs_g = (np.abs(g) + np.abs(f) * np.abs(f * g).sum(-1, keepdims=True)) * inv
        g = (g - f * dot) * inv
    return loss, g, (df * df).sum(-1).mean(), abs_g


BWD_LENS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 77, 79, 80, 81, 95, 96]   # every tile count, each boundary +- 1


def attn_bwd_pack(seed, lens, heads, ft, gt):
    """One pack of sequences for the attention backward: standard normal q|k|v [sum(lens), 3d] rounded to ft and dO [sum(lens), d]
    rounded to gt (float64 arrays), with the float64 reference and the rounding model of every sequence, concatenated."""
    rng = np.random.default_rng(seed)
    rows, d = int(sum(lens)), heads * 64
    qkv = round16(rng.standard_normal((rows, 3 * d)).astype(np.float32), ft)
    do = round16(rng.standard_normal((rows, d)).astype(np.float32), gt)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    exact = np.concatenate([attn_bwd_seq_ref(qkv[a:b], do[a:b], heads, ft, gt) for a, b in zip(cu[:-1], cu[1:])])
    model = np.concatenate([attn_bwd_seq_ref(qkv[a:b], do[a:b], heads, ft, gt, model=True) for a, b in zip(cu[:-1], cu[1:])])
    return qkv, do, exact, model
