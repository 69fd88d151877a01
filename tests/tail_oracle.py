"""A local float64 restatement of the kernels every train step ends in (csrc/kernels_head.hip.h, kernels_tail.hip.h, adam_kernel
of kernels_bwd.hip.h), for tests/tail_sweep.py.

The whole-step oracle (engine_checks.check_train_steps) has to impose the engine's ReLU decisions and to loosen its bounds,
because the errors of the blocks reach the head.  These kernels can be isolated instead: after an engine step the test reads the
engine's OWN inputs of the head - p_L (debug_read "p<L>"; bf16 storage is widened exactly), BN_L's folded rows (debug_read
"bn<L>": scale, shift, mean, rstd), the dense kernel and bias, the labels and weights it set - and everything below is computed
from those alone, in numpy float64.

ReLU decisions need no imposition: the engine decides on fmaf(raw, scale, shift) > 0 in float32.  raw * scale is a product of two
24-bit significands, exact in float64's 53; adding shift rounds once, and a correctly rounded sum has the sign of the exact sum (it
is zero only if the exact sum is).  The float32 fma rounds that same exact value, so its sign is the same again.  activations()
asserts that the float64 decision and the decision on the value rounded to float32 never differ.

Bounds are derived, not tuned.  A float32 sum evaluated as a tree of depth d over terms t_i errs by at most d * 2^-24 * sum |t_i| to
first order; every bound below is TWICE that (the factor 2 covers the float32 rounding of the terms themselves: at most three
roundings per term against d >= 3), with d read from the code - the line is quoted next to each d.  Probabilities, losses and dz
follow from z through expf: the z bound is propagated through the float64 derivative (its supremum over [z - bz, z + bz]) plus
4 ulp for expf and the division."""
import numpy as np

U = 2.0 ** -24                 # float32 unit roundoff
K_THREADS = 256                # kThreads
K_DENSE_CHUNKS = 32            # kDenseChunks (engine.hip.h)
K_FINAL_SLICES = 8             # kFinalSlices = kThreads / kFinalCols (kernels_tail.hip.h)
KERAS_LO = float(np.float32(1e-7))                     # kKerasEps
KERAS_HI = float(np.float32(1.0) - np.float32(1e-7))   # 1.0f - kKerasEps


def head_groups(C):
    """NRG of head_kernel<C, ...>: frame groups of a workgroup (kThreads / (C / 4)); 256 % (C / 4) threads idle."""
    return K_THREADS // (C // 4)


# ------------------------------------------------------------------------------------------ activations
def activations(p, scale, shift, res=None):
    """relu(bn(p_L)) [B, T, C] in float64 and the ReLU decisions, from the engine's p_L and BN_L's folded scale / shift rows.
    `res` = (rp [B, T, C] (already dropped to the last frames), rscale, rshift): the residual branch added before the ReLU
    (dense_grad_body RES form: fmaxf(fmaf(v, sc, sh) + fmaf(r, rsc, rsh), 0)).  Returns (a, decisions, slack) - slack [B, T, C] is
    |main| + |residual| where a residual is added (the float32 sum of two rounded values errs relative to those, not to a), else 0."""
    pre = p.astype(np.float64) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    if res is None:
        dec = pre > 0
        assert np.array_equal(dec, pre.astype(np.float32) > 0), "a ReLU decision differs between float64 and float32"
        return np.where(dec, pre, 0.0), dec, np.zeros_like(pre)
    rp, rsc, rsh = res
    r = rp.astype(np.float64) * np.asarray(rsc, np.float64) + np.asarray(rsh, np.float64)
    # the engine adds the two float32-rounded values in float32: that sum's sign is the sign of their exact sum
    s32 = pre.astype(np.float32).astype(np.float64) + r.astype(np.float32).astype(np.float64)
    dec = s32 > 0
    assert np.array_equal(dec, s32.astype(np.float32) > 0), "a ReLU decision differs between float64 and float32"
    return np.where(dec, pre + r, 0.0), dec, np.abs(pre) + np.abs(r)


# ------------------------------------------------------------------------------------------ logit, probability, loss, dz
def _sigmoid(z):
    return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


def _dsig_sup(z, bz):
    """sup of sigmoid' over [z - bz, z + bz]: p (1 - p) peaks at 0"""
    lo, hi = z - bz, z + bz
    s = np.maximum(_sigmoid(lo) * (1 - _sigmoid(lo)), _sigmoid(hi) * (1 - _sigmoid(hi)))
    return np.where((lo <= 0) & (hi >= 0), 0.25, s)


def head(a, wd, bd, y, w, J, clipped=False):
    """The head of one batch from its activations a [B, T, C] (float64): z, p, the weighted loss (sum_i w_i bce_i / B), dz and
    their bounds.  J: the JMAX of the head_kernel instantiation that runs (its dot product is a chain of 4 * JMAX fmas whatever T).
    y / w None: a forward without labels (z and p only)."""
    B = a.shape[0]
    terms = a * np.asarray(wd, np.float64).reshape(a.shape[1:])
    z = terms.sum(axis=(1, 2)) + float(bd)
    # depth of z (head_kernel):  "for j < JMAX: dot = fmaf(.x) fmaf(.y) fmaf(.z) fmaf(.w)"   4 * J
    #                            "dot = wave_sum(dot)"                                       6 shuffle levels of a 64-lane wave
    #                            "((sRed[0] + sRed[1]) + (sRed[2] + sRed[3])) + bias"        2 levels over the wave partials + 1
    d_z = 4 * J + 6 + 2 + 1
    bz = 2 * d_z * U * (np.abs(terms).sum(axis=(1, 2)) + abs(float(bd)))
    p = _sigmoid(z)
    # p = 1 / (1 + expf(-z)): the z bound through sigmoid', + 4 ulp (expf, the addition, the division)
    bp = _dsig_sup(z, bz) * bz + 4 * np.spacing(np.maximum(p, 1e-37).astype(np.float32)).astype(np.float64)
    out = dict(z=z, bz=bz, p=p, bp=bp, terms=terms, d_z=d_z)
    if y is None:
        return out
    y = np.asarray(y, np.float64)
    w = np.asarray(w, np.float64)
    if clipped:
        # bce_value clipped form: -(y logf(pc) + (1 - y) logf(1 - pc)), pc = clip(p, eps, 1 - eps); bce_dz = 0 outside the clip
        assert np.all((np.abs(p - KERAS_LO) > 2 * bp) & (np.abs(p - KERAS_HI) > 2 * bp)), "a probability within its bound of the Keras clip"
        inside = (p > KERAS_LO) & (p < KERAS_HI)
        pc = np.clip(p, KERAS_LO, KERAS_HI)
        bce = -(y * np.log(pc) + (1 - y) * np.log(1 - pc))
        # d bce / d p = -y / pc + (1 - y) / (1 - pc) inside the clip, 0 outside; 1.0f - pc rounds once (2^-24 absolute);
        # logf and the combination: 4 ulp of the value
        bbce = np.where(inside, bp * (y / pc + (1 - y) / (1 - pc)), 0.0) + (1 - y) * U / (1 - pc) + 4 * U * np.abs(bce)
        dzr = np.where(inside, p - y, 0.0)
        bdzr = np.where(inside, bp, 0.0)
    else:
        # bce_value logits form: fmaxf(z, 0) - z y + log1pf(expf(-|z|)); |d / dz| = |sigmoid(z) - y| <= 1; the three terms are
        # bounded by |z|, |z|, log 2 and are combined in two roundings, expf and log1pf err by 2 ulp each
        bce = np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z)))
        bbce = bz + 4 * U * (np.abs(z) + 1.0)
        dzr = p - y
        bdzr = bp
    loss_i = w * bce / B
    # loss_part = w * bce * inv_b and dz = w * bce_dz * inv_b: inv_b = 1.0f / (float)B and two products (+ the subtraction
    # pr - yy): 4 roundings relative to the value
    bloss_i = np.abs(w) / B * bbce + 4 * U * np.abs(loss_i)
    dz = w * dzr / B
    bdz = np.abs(w) / B * bdzr + 4 * U * np.abs(dz)
    loss = float(loss_i.sum())
    out.update(bce=bce, loss=loss, bloss=float(bloss_i.sum()) + U * abs(loss), dz=dz, bdz=bdz)   # (+ the float cast of the host's double sum)
    return out


def head_input_condition(h):
    """Dropping the largest term of any one final frame row moves z by more than twice its bound in at least one window
    (a case that cannot see a lost row is not a test).  Returns the frame rows that fail."""
    big = np.abs(h["terms"]).max(axis=2)                      # [B, T]
    seen = (big > 2 * h["bz"][:, None]).any(axis=0)
    return np.nonzero(~seen)[0]


# ------------------------------------------------------------------------------------------ dense-weight gradient
def dense_chunks(B):
    """(chunk, number of chunks, chunks per slice) of the dense-weight gradient at batch B (dense_args, grad_final_kernel)."""
    chunk = -(-B // K_DENSE_CHUNKS)
    n = -(-B // chunk)
    return chunk, n, -(-n // K_FINAL_SLICES)


def dense_grad(a, dz, keep=None, slack=None):
    """dW_dense[e] = sum_b dz_b keep_b[e] a_b[e], db = sum_b dz_b and their bounds, from the engine's own dz (float32, widened)."""
    B = a.shape[0]
    dz = np.asarray(dz, np.float64)
    t = a.reshape(B, -1) * dz[:, None]
    if keep is not None:
        t = t * np.asarray(keep, np.float64).reshape(B, -1)
    chunk, n, per = dense_chunks(B)
    # depth (dense_role_chunks / dense_grad_body + grad_final_kernel):
    #   "sub = fmaf(dz[u], fmaxf(...), sub)" over the rows of a chunk              chunk
    #   "acc += sub" over the chunks of a slice (route B: "acc += v[u]" over the slice's partial rows)   per
    #   "for j < kFinalSlices: g += sSum[j * kFinalCols + pl]"                     kFinalSlices
    d = chunk + per + K_FINAL_SLICES
    bw = 2 * d * U * np.abs(t).sum(axis=0)
    if slack is not None:   # RES: fmaf(r, rsc, rsh), fmaf(v, sc, sh) and their sum round relative to |main| + |residual|
        bw = bw + 3 * U * (np.abs(dz)[:, None] * (slack.reshape(B, -1) if keep is None else slack.reshape(B, -1) * np.abs(np.asarray(keep, np.float64).reshape(B, -1)))).sum(axis=0)
    # bias: "sub += d.dz[b]" / "s += a.dz[b]" over a chunk, the chunks of a slice, the slices
    bb = 2 * d * U * np.abs(dz).sum()
    return dict(dW=t.sum(axis=0), bW=bw, db=float(dz.sum()), bdb=float(bb), terms=t, d=d)


def dense_input_condition(g, live):
    """Dropping any one window moves at least one dense-gradient element by more than twice its bound.  `live`: windows whose
    dz is not zero by construction (a zero sample weight contributes exactly nothing: there is nothing to lose).  Returns the
    windows that fail."""
    seen = (np.abs(g["terms"]) > 2 * g["bW"][None, :]).any(axis=1)
    return np.nonzero(~seen & np.asarray(live, bool))[0]


# ------------------------------------------------------------------------------------------ BN_L backward sums
def bn_sums(p, mean, rstd, dec, wd, dz, J, windows_per_wg):
    """BN_L's d gamma = sum g xhat and d beta = sum g with g = dz_b wd[t, c] relu'(.), xhat = (raw - mean) rstd, and their bounds."""
    B, T, C = p.shape
    g = np.where(dec, np.asarray(dz, np.float64)[:, None, None] * np.asarray(wd, np.float64).reshape(T, C), 0.0)
    gx = g * ((p.astype(np.float64) - np.asarray(mean, np.float64)) * np.asarray(rstd, np.float64))
    # depth (head_kernel):  "g1.x += gx" / "g2.x = fmaf(gx, ..., g2.x)" over JMAX rows of every window of the workgroup   J * windows
    #                       "for r < NRG: v += sStat[r * 2 * C + tid]"                                                    NRG
    #                       the rows are folded in double (publish_stat / reduce_partials_256), one cast "(float)s1"      1
    d = J * windows_per_wg + head_groups(C) + 1
    return dict(dbeta=g.sum(axis=(0, 1)), bdbeta=2 * d * U * np.abs(g).sum(axis=(0, 1)),
                dgamma=gx.sum(axis=(0, 1)), bdgamma=2 * d * U * np.abs(gx).sum(axis=(0, 1)), d=d)


# ------------------------------------------------------------------------------------------ Adam
BETA1, BETA2, EPS = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-7))   # the float32 constants of the kernel


def _libm_powf():
    import ctypes
    import ctypes.util
    f = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").powf
    f.restype, f.argtypes = ctypes.c_float, (ctypes.c_float, ctypes.c_float)
    return f


_powf = _libm_powf()


def adam_alpha(lr, t):
    """adam_alpha of mww_lib.hip: Keras's alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t) evaluated in float32 on the host (1 - beta2^t
    cancels: a float64 evaluation differs by up to 2^-24 / (1 - beta2^t), 3e-5 at t = 2 - the host's float32 value is the
    definition here, as it is in Keras).  powf is the C library's, the very function the host code calls: numpy's float32 power
    is an implementation of its own and differs from it by one ulp now and then (t = 9: 3e-6 of alpha after the cancellation);
    sqrtf, the subtraction and the division are correctly rounded everywhere."""
    f = np.float32
    b1p, b2p = f(_powf(0.9, float(t))), f(_powf(0.999, float(t)))
    return float(f(lr) * np.sqrt(f(1.0) - b2p) / (f(1.0) - b1p))


def adam_step(param, m, v, grad, lr, t, gscale=1.0):
    """One Keras-Adam update (oracle.model_oracle.KerasAdam's arithmetic, epsilon outside the root) in float64 from the engine's
    own float32 state and gradient; returns (param, m, v, bound).  The update expression rounds five times -
        m += (g - m) (1 - beta1)      v += (g g - v) (1 - beta2)      sqrtf(v) + eps      alpha m / (.)      param -= .
    each of the first four is made of at most three float32 operations whose results are bounded by |update| relative to the
    final quotient (<= 3 * 4 = 12 roundings of 2^-24 |update|, the root halves v's share), the last rounds relative to
    |param| + |update|; alpha and hyper[1] carry one more each: 16 * 2^-24 * (|param| + |update|) covers them."""
    param, m, v, g = (np.asarray(x, np.float64) for x in (param, m, v, grad))
    gg = g * float(np.float32(gscale))
    m2 = m + (gg - m) * (1.0 - BETA1)
    v2 = v + (gg * gg - v) * (1.0 - BETA2)
    upd = adam_alpha(lr, t) * m2 / (np.sqrt(v2) + EPS)
    return param - upd, m2, v2, 16 * U * (np.abs(param) + np.abs(upd))
