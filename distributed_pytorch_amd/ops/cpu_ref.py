"""Plain-PyTorch reference implementation of the native kernel API (same names, same signatures,
same in-place output semantics as ``distributed_pytorch_amd._C``).

Used (a) as the CPU backend of the training engine, so the whole distributed harness — sync
modes, buckets, checkpointing — runs and is tested on CPU with gloo, and (b) as the numerics
oracle the HIP kernels are checked against.  Tensors follow the native layouts: NHWC
activations, KRSC conv weights.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

CHUNK = 64


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


# ---------------------------------------------------------------- optimizer / elementwise
def _rate(lr):
    """The rate of the update functions: a float, or the value of a 1-element tensor."""
    return float(lr[0]) if torch.is_tensor(lr) else lr


def sgd_flat(p, g, buf, lr, momentum, wd, gscale, first, offset=0, count=-1, planes=None):
    lr = _rate(lr)
    if count < 0:
        count = p.numel() - offset
    sl = slice(offset, offset + count)
    pp, gg, bb = p[sl], g[sl], buf[sl]
    d = gg * gscale + wd * pp
    if first:
        bb.copy_(d)
    else:
        bb.mul_(momentum).add_(d)
    pp.sub_(lr * bb)
    if planes is not None:
        planes[:, sl].copy_(split_bf16(pp, planes.shape[0]))


OPT_CHUNK = 8192  # chunk length of the optimizer's block map (kernels/lars.hip)


def sqnorm_partials(p, g, bmap, partials, nseg):
    """partials[b] = (sum p^2, sum g^2) of chunk b in fp64 (bmap: utils/arena.block_map)."""
    out = partials.view(-1, 2)
    for b, (seg, start, ln) in enumerate(bmap.tolist()):
        out[b, 0] = p[start:start + ln].double().square().sum()
        out[b, 1] = g[start:start + ln].double().square().sum()


def lars_finalize(partials, segs, table, stats, gscale, max_norm, trust_coef, wd, eps):
    """Per-segment norms from the chunk partials, the clip coefficient (clip_grad_norm_ of the
    scaled gradient) and the LARS trust ratios, all in fp64 (kernels/lars.hip (b)).
    table: r_s per segment, then gmul = gscale * c.  stats: |p|_s, gscale |g|_s, gscale |g|, c."""
    part = partials.view(-1, 2).double()
    rows = segs.tolist()
    S = len(rows)
    P = [float(part[f:f + c, 0].sum()) for f, c, _ in rows]
    Gs = [float(part[f:f + c, 1].sum()) for f, c, _ in rows]
    G = 0.0
    for v in Gs:
        G += v
    gnorm = gscale * math.sqrt(G)
    c = min(1.0, max_norm / (gnorm + 1e-6)) if max_norm > 0 else 1.0
    gmul = gscale * c
    for s, (_, _, adapt) in enumerate(rows):
        pn, gn = math.sqrt(P[s]), gmul * math.sqrt(Gs[s])
        r = trust_coef * pn / (gn + wd * pn + eps) if adapt and pn > 0 and gn > 0 else 1.0
        table[s] = r
        stats[s] = pn
        stats[S + s] = gscale * math.sqrt(Gs[s])
    table[S] = gmul
    stats[2 * S] = gnorm
    stats[2 * S + 1] = c


def sgd_segmented(p, g, buf, bmap, table, lr, momentum, wd, first, planes=None):
    """sgd_flat over the chunks of bmap with the segment's trust ratio and the table's gradient
    multiplier:  d = (g * gmul + wd * p) * r_s ; buf = first ? d : momentum * buf + d ; p -= lr * buf
    (LARS with the learning rate outside the momentum, as apex LARC / torchlars)."""
    lr = _rate(lr)
    S = table.numel() - 1
    gmul = table[S].to(p.dtype)
    r = torch.ones_like(p)
    cov = torch.zeros(p.numel(), dtype=torch.bool)
    for seg, start, ln in bmap.tolist():
        r[start:start + ln] = table[seg].to(p.dtype)
        cov[start:start + ln] = True
    d = (g * gmul + wd * p) * r
    nb = d if first else buf * momentum + d
    if bool(cov.all()):
        buf.copy_(nb)
        p.sub_(lr * buf)
    else:
        buf[cov] = nb[cov]
        p[cov] = p[cov] - lr * buf[cov]
    if planes is not None:
        pl = split_bf16(p, planes.shape[0])
        planes[:, cov] = pl[:, cov]


def grad_fold(acc, g, mode, offset=0, count=-1):
    """kernels/grad_fold.hip over [offset, offset + count) of two flat fp32 arenas:
    mode 0 store: acc = g   1 add: acc = acc + g   2 merge: g = acc + g (plain ``torch.add``)."""
    for t in (acc, g):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError("grad_fold: acc and g must be float32 tensors")
        if not t.is_contiguous():
            raise ValueError("grad_fold: acc and g must be contiguous")
    if acc.device != g.device:
        raise ValueError("grad_fold: acc and g must be on one device")
    if acc.numel() != g.numel():
        raise ValueError("grad_fold: acc and g must have one length")
    if mode not in (0, 1, 2):
        raise ValueError("grad_fold: mode must be 0 (store), 1 (add) or 2 (merge)")
    if offset < 0:
        raise ValueError("grad_fold: offset must be >= 0")
    if count < -1:
        raise ValueError("grad_fold: count must be >= 0 (or -1: to the end)")
    if offset > acc.numel():
        raise ValueError("grad_fold: the slice ends past the arena")
    if count < 0:
        count = acc.numel() - offset
    if offset % 4 or count % 4:
        raise ValueError("grad_fold: offset and count must be multiples of 4")
    if count > acc.numel() - offset:
        raise ValueError("grad_fold: the slice ends past the arena")
    a, b = acc.view(-1)[offset:offset + count], g.view(-1)[offset:offset + count]
    if mode == 0:
        a.copy_(b)
    elif mode == 1:
        torch.add(a, b, out=a)
    else:
        torch.add(a, b, out=b)


def lr_advance(table, step, lr, host_pos, from_device):
    """kernels/lr_sched.hip: lr[0] = table[min(pos, T - 1)], step[0] = pos + 1, with pos the
    counter's value (from_device) or host_pos."""
    pos = int(step[0]) if from_device else int(host_pos)
    lr[0] = table[min(max(pos, 0), table.numel() - 1)]
    step[0] = pos + 1


def split_bf16(x, np_):
    """fp32 -> [np_, *x.shape] bf16 planes (round-to-nearest-even), the HIP split's semantics."""
    out, r = [], x.float()
    for _ in range(np_):
        h = r.to(torch.bfloat16)
        out.append(h)
        r = r - h.float()
    return torch.stack(out)


def mean_of_w(inp, out, W):
    out.copy_(inp.view(W, -1).mean(0))


# ---------------------------------------------------------------- convolution
def conv_splits(Kred, splits):
    return max(1, min(max(1, splits), -(-Kred // 32)))


def conv_fprop(x, w, out, slab, stride, pad, splits=1, tile=0, dgrad=False, reduce=True, posmajor=False):
    if dgrad:  # w: the original conv's weights [C_in_of_this_gemm=K_orig, R, S, C_orig]
        w = w.flip(1, 2).permute(3, 1, 2, 0)
    y = _nhwc(F.conv2d(_nchw(x), _nchw(w), stride=stride, padding=pad))
    eff = conv_splits(w.shape[1] * w.shape[2] * w.shape[3], splits)
    if eff > 1 and not reduce:  # mirror the native contract: the slabs sum to the result
        n = y.numel()
        slab[:eff * n].zero_()
        slab[:n].copy_(y.reshape(-1))
        return
    out.copy_(y)


def conv_wgrad(x, dz, dw, slab, stride, pad, splits=1, tile=0, posmajor=False):
    K, R, S, C = dw.shape
    gw = torch.nn.grad.conv2d_weight(_nchw(x), (K, C, R, S), _nchw(dz), stride=stride, padding=pad)
    dw.copy_(_nhwc(gw))


def wflip(w, wd):
    wd.copy_(w.flip(1, 2).permute(3, 1, 2, 0))


# ---------------------------------------------------------------- batch norm
def bn_part_floats(M, C, bwd):
    return (3 if bwd else 2) * C * ((M + CHUNK - 1) // CHUNK)


def bn_fwd_stats(src, nsplit, z, part, gamma, beta, bias, rmean, rvar, nbt, mean, invstd, scale, shift, momentum,
                 eps):
    C = z.shape[-1]
    if nsplit > 1:
        z.copy_(src[:nsplit * z.numel()].view(nsplit, -1).sum(0).view(z.shape))
    zz = z.reshape(-1, C).double()
    n = zz.shape[0]
    mu = zz.mean(0)
    var = zz.var(0, unbiased=False)
    iv = torch.rsqrt(var + eps)
    mean.copy_(mu)
    invstd.copy_(iv)
    scale.copy_(gamma.double() * iv)
    shift.copy_(beta.double() - mu * gamma.double() * iv)
    if rmean is not None:
        b = bias.double() if bias is not None else 0.0
        unb = var * n / max(n - 1, 1)
        rmean.copy_((1 - momentum) * rmean.double() + momentum * (mu + b))
        rvar.copy_((1 - momentum) * rvar.double() + momentum * unb)
    if nbt is not None:
        nbt.add_(1)


def bn_eval_params(gamma, beta, bias, rmean, rvar, scale, shift, eps):
    s = gamma * torch.rsqrt(rvar + eps)
    scale.copy_(s)
    b = bias if bias is not None else 0.0
    shift.copy_(beta + (b - rmean) * s)


def _act(u, act, res):
    if act == 1:
        return u
    if act == 2:
        u = u + res.reshape(u.shape)
    return torch.relu(u)


def bn_apply(z, a, scale, shift, pool, act=0, res=None, mask=None):  # mask: native only (CPU keeps res)
    y = _act(z * scale + shift, act, res)
    if pool:
        y = _nhwc(F.max_pool2d(_nchw(y), 2, 2))
    a.copy_(y.reshape(a.shape))


def bn_bwd(gsrc, nsplit, g, z, scale, shift, mean, invstd, gamma, part, coef, dgamma, dbeta, dbias, dz, pool,
           act=0, res=None, dres=None, sig=None, sig_val=0, g2=None, mask=None):
    N, H, W, C = z.shape
    if nsplit > 1:
        g.copy_(gsrc[:nsplit * g.numel()].view(nsplit, -1).sum(0).view(g.shape))
    else:
        g = gsrc
    if g2 is not None:  # a second contribution to the same gradient (native: summed on load)
        g = g + g2
    with torch.enable_grad():
        u = (z * scale + shift).detach().requires_grad_(True)  # BN output, pre-activation
        y = _act(u, act, res)
        if pool:
            y = _nhwc(F.max_pool2d(_nchw(y), 2, 2))
        (dy,) = torch.autograd.grad(y, u, g.reshape(y.shape))
    if act == 2:
        dres.copy_(dy.reshape(dres.shape))
    xh = (z - mean) * invstd
    M = N * H * W
    sdy = dy.reshape(-1, C).sum(0)
    sdx = (dy * xh).reshape(-1, C).sum(0)
    sx = xh.reshape(-1, C).sum(0)
    k1 = gamma * invstd
    out = k1 * (dy - sdy / M - xh * sdx / M)
    dz.copy_(out)
    dgamma.copy_(sdx)
    dbeta.copy_(sdy)
    if dbias is not None:
        dbias.copy_(-k1 * sx * sdx / M)


def wgrad0_part_floats(N):
    return 1


def bn_bwd_wgrad0(gsrc, nsplit, g, z, scale, shift, mean, invstd, gamma, part, coef, dgamma, dbeta, dbias, x, wpart,
                  dw):
    """Layer-0 backward (native: bn.hip bn_bwd_wgrad0_kernel): BN backward with ReLU + 2x2 max-pool
    routing, then the 3x3/s1/p1 weight gradient on the input x [N,H,W,4] (channels >= 3 zero)."""
    dz = torch.empty_like(z)
    bn_bwd(gsrc, nsplit, g, z, scale, shift, mean, invstd, gamma, part, coef, dgamma, dbeta, dbias, dz, True)
    cin = 3
    w = torch.nn.grad.conv2d_weight(_nchw(x[..., :cin]), (z.shape[-1], cin, 3, 3), _nchw(dz), padding=1)
    dw.zero_()
    dw[..., :cin].copy_(w.permute(0, 2, 3, 1))


# ---------------------------------------------------------------- classifier head
def fc_ce_train(x, w, b, target, loss_row, dlogits, dx, dw, db, loss_out, loss_accum, bn_z=None, bn_scale=None,
                bn_shift=None, label_smoothing=0.0, target2=None, lam=None):
    """Linear + softmax cross-entropy (mean), forward and backward (native: fc_ce.hip).  With
    label_smoothing eps (torch's F.cross_entropy(label_smoothing=eps)):
    loss_row = lse(z) - (1 - eps) z_t - (eps / J) sum_j z_j,
    dlogits_j = (softmax_j - (1 - eps) [j == t] - eps / J) / B.
    With pair targets (Mixup / CutMix: target2 int64 [B] and lam [B], both or neither) the one-hot
    target is q = lam onehot(target) + (1 - lam) onehot(target2):
    loss_row = lse(z) - (1 - eps) (lam z_t1 + (1 - lam) z_t2) - (eps / J) sum_j z_j,
    dlogits_j = (softmax_j - (1 - eps) q_j - eps / J) / B."""
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise ValueError("label_smoothing must be in [0, 1)")
    if (target2 is None) != (lam is None):
        raise ValueError("target2 and lam must be given together")
    B = x.shape[0]
    if bn_z is not None:  # features from the last conv's z: BN + ReLU + 2x2 max-pool, written to x
        x.copy_(torch.relu(bn_z * bn_scale + bn_shift).reshape(B, 4, -1).amax(1))
    logits = x @ w.t() + b
    lse = torch.logsumexp(logits, 1)
    p = torch.softmax(logits, 1)
    if target2 is not None:
        la = lam.to(logits.dtype)
        zt = la * logits.gather(1, target.view(-1, 1)).squeeze(1) \
            + (1.0 - la) * logits.gather(1, target2.view(-1, 1)).squeeze(1)
        lr = lse - (1.0 - eps) * zt - eps * logits.mean(1)
        q = torch.zeros_like(p)
        q[torch.arange(B), target] += la
        q[torch.arange(B), target2] += 1.0 - la
        p -= (1.0 - eps) * q + eps / logits.shape[1]
        p /= B
    else:
        lr = lse - logits.gather(1, target.view(-1, 1)).squeeze(1)
        if eps:
            lr = lse - (1.0 - eps) * logits.gather(1, target.view(-1, 1)).squeeze(1) - eps * logits.mean(1)
        p[torch.arange(B), target] -= 1.0 - eps
        if eps:
            p -= eps / logits.shape[1]
        p /= B
    loss_row.copy_(lr)
    dlogits.copy_(p.reshape(dlogits.shape))
    dx.copy_(p @ w)
    dw.copy_(p.t() @ x)
    db.copy_(p.sum(0))
    l = lr.mean()
    loss_out.reshape(-1)[0] = l
    if loss_accum is not None:
        loss_accum.reshape(-1)[0] += l


def fc_ce_eval(x, w, b, target, loss_row, correct_row, logits=None, acc=None):
    lg = x @ w.t() + b
    lse = torch.logsumexp(lg, 1)
    lr = lse - lg.gather(1, target.view(-1, 1)).squeeze(1)
    loss_row.copy_(lr)
    correct_row.copy_((lg.argmax(1) == target).to(correct_row.dtype))
    if logits is not None:
        logits.copy_(lg)
    if acc is not None:
        acc[0] += lr.mean()
        acc[1] += correct_row.sum().to(acc.dtype)


# ---------------------------------------------------------------- data
_M1 = 0x9E3779B97F4A7C15
_M2 = 0xBF58476D1CE4E5B9
_M3 = 0x94D049BB133111EB
_MASK = (1 << 64) - 1


def _mix64(z):
    z = (z + _M1) & _MASK
    z = ((z ^ (z >> 30)) * _M2) & _MASK
    z = ((z ^ (z >> 27)) * _M3) & _MASK
    return z ^ (z >> 31)


def aug_params(seed, salt, b, pad):
    """(dy, dx, flip) of sample slot b — bit-identical to the HIP kernel's hash."""
    h = _mix64((seed & _MASK) ^ _mix64((salt * 0x100000001B3 + b) & _MASK))
    span = 2 * pad + 1
    return h % span, (h >> 16) % span, (h >> 40) & 1


def augment(images, idx, labels, out, target, pad, train, seed, salt, mean, std):
    B = idx.numel()
    Hs, Ws = images.shape[1], images.shape[2]
    m = torch.tensor(mean, dtype=torch.float32)
    inv = 1.0 / torch.tensor(std, dtype=torch.float32)
    src = images[idx.long()].float() * (1.0 / 255.0)  # B H W 3
    res = torch.zeros(B, Hs, Ws, 4)
    for b in range(B):
        if train:
            dy, dx, flip = aug_params(seed, salt, b, pad)
        else:
            dy, dx, flip = pad, pad, 0
        padded = torch.zeros(Hs + 2 * pad, Ws + 2 * pad, 3)
        padded[pad:pad + Hs, pad:pad + Ws] = src[b]
        crop = padded[dy:dy + Hs, dx:dx + Ws]
        if flip:
            crop = crop.flip(1)
        res[b, :, :, :3] = (crop - m) * inv
    out.copy_(res.reshape(out.shape))
    if target is not None:
        target.copy_(labels[idx.long()])


MIXUP, CUTMIX = 0, 1
# The hash input of a batch's mix parameters takes the place of a slot index in aug_params' input
# salt * 0x100000001B3 + b.  Slot indices are block indices of one launch, below 2^31; 2^32 - 1 is
# none of them, so the mix stream never coincides with a sample's crop / flip stream of the same
# (seed, salt).
MIX_SLOT = 0xFFFFFFFF


def mix_params(seed, salt, mode, alpha, Hs, Ws):
    """(lam, y0, y1, x0, x1) of one batch's Mixup (mode 0) or CutMix (mode 1): pure Python, a
    function of (seed, salt) alone, the one source of mix parameters for both loader backends.
    lam0 ~ Beta(alpha, alpha).  Mixup: lam = lam0, empty box.  CutMix (the paper's rand_bbox): a
    box of area share ~(1 - lam0) around a uniform centre, clipped to the image; lam = 1 - the
    box's exact area share."""
    import random

    if not alpha > 0:
        raise ValueError(f"mix alpha must be > 0, got {alpha!r}")
    if mode not in (MIXUP, CUTMIX):
        raise ValueError("mode must be 0 (Mixup) or 1 (CutMix)")
    h = _mix64((seed & _MASK) ^ _mix64((salt * 0x100000001B3 + MIX_SLOT) & _MASK))
    r = random.Random(h)
    lam0 = r.betavariate(alpha, alpha)
    if mode == MIXUP:
        return lam0, 0, 0, 0, 0
    cy, cx = r.randrange(Hs), r.randrange(Ws)
    cut = math.sqrt(1.0 - lam0)
    ch, cw = int(Hs * cut), int(Ws * cut)
    y0, y1 = max(cy - ch // 2, 0), min(cy + ch // 2, Hs)
    x0, x1 = max(cx - cw // 2, 0), min(cx + cw // 2, Ws)
    return 1.0 - (y1 - y0) * (x1 - x0) / (Hs * Ws), y0, y1, x0, x1


def augment_mix(images, idx, labels, out, target, target2, lam_out, pad, seed, salt, mean, std, mode, lam, y0=0,
                y1=0, x0=0, x1=0):
    """The training ``augment``, then slot b mixed with slot B-1-b (native: augment.hip
    augment_mix_kernel).  Mixup: out = lam aug + (1 - lam) aug.flip(0) in fp32; CutMix: the box
    [y0,y1) x [x0,x1) of aug.flip(0) pasted into aug.  target2 = the partners' labels, lam_out = lam."""
    if mode not in (MIXUP, CUTMIX):
        raise ValueError("mode must be 0 (Mixup) or 1 (CutMix)")
    if not 0.0 <= lam <= 1.0:
        raise ValueError("lam must be in [0, 1]")
    B = idx.numel()
    Hs, Ws = images.shape[1], images.shape[2]
    if mode == CUTMIX and not (0 <= y0 <= y1 <= Hs and 0 <= x0 <= x1 <= Ws):
        raise ValueError("the box must lie inside the image")
    a = torch.zeros(B, Hs, Ws, 4)
    augment(images, idx, labels, a, target, pad, True, seed, salt, mean, std)
    if mode == MIXUP:
        l32 = torch.tensor(lam, dtype=torch.float32)
        res = l32 * a + (1.0 - l32) * a.flip(0)
    else:
        res = a.clone()
        res[:, y0:y1, x0:x1] = a.flip(0)[:, y0:y1, x0:x1]
    out.copy_(res.reshape(out.shape))
    target2.copy_(labels[idx.long()].flip(0))
    lam_out.fill_(lam)
