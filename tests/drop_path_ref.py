"""Host restatements for the stochastic-depth (drop-path) tests: the Philox4x32-10 generator and the keep table that
x3d_drop_path_draw builds from it (include/x3d_hip.h K9d), and the training forward with drop-path on top of the CPU oracle's
own layer functions -- the only change against oracle.x3d_oracle.res_block is `c = keep[l][:, None, None, None, None] * bn_c(c)`."""
import numpy as np
import torch

from oracle import x3d_oracle as O
from oracle.x3d_oracle import Storage, _relu, batch_norm, block_prefix, pointwise, stem  # noqa: F401

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF

# (counter, key) -> output, checked on the CPU when the feature was specified
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((_MASK,) * 4, (_MASK,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(counter, key):
    """Philox4x32-10: counter (c0, c1, c2, c3), key (k0, k1) -> four 32-bit words.  One round is
    c' = (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)); the key is bumped by (W0, W1) between rounds."""
    c0, c1, c2, c3 = (int(v) & _MASK for v in counter)
    k0, k1 = (int(v) & _MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + W0) & _MASK, (k1 + W1) & _MASK
    return c0, c1, c2, c3


def rates32(rates):
    """the per-block rates as the device holds them: fp32"""
    return np.asarray(rates, dtype=np.float64).astype(np.float32)


def keep_scale(rates):
    """fp32(1.0f / (1.0f - rate_l)) per block"""
    return np.float32(1.0) / (np.float32(1.0) - rates32(rates))


def keep_table(seed, step, rates, n):
    """keep [L][N] fp32 of step `step`: key (seed_lo, seed_hi), counter (step_lo, step_hi, l, n), u = (out[0] >> 8) * 2^-24,
    kept iff u >= rate_l (fp32 comparison), kept samples scaled by fp32(1 / (1 - rate_l))."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    r32, sc = rates32(rates), keep_scale(rates)
    out = np.zeros((len(r32), n), dtype=np.float32)
    for l in range(len(r32)):
        for i in range(n):
            w = philox4x32_10((step & _MASK, step >> 32, l, i), (seed & _MASK, seed >> 32))[0]
            u = np.float32((w >> 8) * 2.0 ** -24)
            out[l, i] = sc[l] if u >= r32[l] else np.float32(0.0)
    return out


def scaled_mask(mask01, rates):
    """a [L][N] 0/1 keep mask -> the keep table X3D.set_drop_path_mask builds from it (torch, fp32)"""
    return torch.as_tensor(mask01, dtype=torch.float32) * torch.from_numpy(keep_scale(rates)).view(-1, 1)


def res_block_dp(x, p, b, arch, state, keep, taps=None, masks=None, st=O._FP32):
    """oracle.x3d_oracle.res_block in training mode with the bottleneck branch scaled per sample: keep [N] (0, or 1 / (1 - rate));
    None = the oracle's block.  bn_c still takes its statistics over all samples: the drop sits behind it."""
    if keep is None:
        return O.res_block(x, p, b, arch, True, state, taps, masks, st)
    pre = block_prefix(b)
    q = f"{pre}/bottleneck"
    eps, mom = arch.bn_eps, arch.bn_momentum
    a = st.act(pointwise(x, p[f"{q}/a/kernel"]))
    a_act = _relu(st.grad(batch_norm(a, p, f"{q}/bn_a", True, eps, mom, state)), f"{pre}/a", masks)
    bb = st.act(st.depthwise(a_act, p[f"{q}/b/kernel"], b.stride, pre))
    u = batch_norm(bb, p, f"{q}/bn_b", True, eps, mom, state)
    if b.has_se:
        pooled = u.mean((2, 3, 4))
        s1 = _relu(pooled @ p[f"{q}/se_fc1/kernel"].t() + p[f"{q}/se_fc1/bias"], f"{pre}/se", masks)
        gate = torch.sigmoid(s1 @ p[f"{q}/se_fc2/kernel"].t() + p[f"{q}/se_fc2/bias"])
        u = u * gate[:, :, None, None, None]
    u = st.grad(u)
    s = u * torch.sigmoid(u)
    c = st.act(pointwise(s, p[f"{q}/c/kernel"]))
    c = batch_norm(c, p, f"{q}/bn_c", True, eps, mom, state)
    c = keep.to(c.dtype)[:, None, None, None, None] * c            # <- stochastic depth
    if b.has_shortcut_conv:
        xs = x[:, :, :, ::b.stride, ::b.stride] if b.stride != 1 else x
        r = st.act(pointwise(st.grad(xs), p[f"{pre}/residual/kernel"]))
        r = batch_norm(r, p, f"{pre}/bn_r", True, eps, mom, state)
    else:
        r = x
    y = st.grad(st.act(_relu(r + c, f"{pre}/out", masks)))
    if taps is not None:
        taps[f"{pre}/a_raw"] = a
        taps[f"{pre}/b_raw"] = bb
        taps[f"{pre}/out"] = y
    return y


def forward_dp(p, x_nthwc, arch, keep, rates, dropout_mask=None, state=None, taps=None, relu_masks=None, storage=None):
    """oracle.x3d_oracle.forward(training=True) with drop-path: keep [L][N] (already scaled); blocks with rate 0 run the
    oracle's own block.  Returns the probabilities [N, classes]."""
    st = storage if isinstance(storage, Storage) else Storage(storage)
    x = st.act(x_nthwc.permute(0, 4, 1, 2, 3))
    out = stem(x, p, arch, True, state, relu_masks, st)
    if taps is not None:
        taps["conv1/out"] = out
    for l, b in enumerate(arch.blocks):
        out = res_block_dp(out, p, b, arch, state, keep[l] if rates[l] > 0 else None, taps, relu_masks, st)
    out = st.act(pointwise(out, p["conv5/layer_with_weights-0/kernel"]))
    out = _relu(st.grad(batch_norm(out, p, "conv5/layer_with_weights-1", True, arch.bn_eps, arch.bn_momentum, state)),
                "conv5", relu_masks)
    pooled = out.mean((2, 3, 4))
    h = _relu(pooled @ p["fc1/kernel"].t(), "fc1", relu_masks)
    if arch.dropout_rate > 0:
        h = h * dropout_mask / (1.0 - arch.dropout_rate)
    logits = h @ p["fc2/kernel"].t() + p["fc2/bias"]
    if taps is not None:
        taps["logits"] = logits
    return torch.softmax(logits.float(), -1).reshape(-1, arch.num_classes)


def train_step_dp(p, x_nthwc, labels, arch, keep, rates, dropout_mask=None, relu_masks=None, taps=None):
    """oracle.x3d_oracle.train_step (no update) over forward_dp: dict(loss, probs, grads, state)."""
    names = O.trainable_names(p)
    leaf = {k: (v.detach().clone().requires_grad_(True) if k in names else v) for k, v in p.items()}
    state = O.BNState()
    probs = forward_dp(leaf, x_nthwc, arch, keep, rates, dropout_mask=dropout_mask, state=state, taps=taps, relu_masks=relu_masks)
    loss, ce, reg = O.loss_fn(probs, labels, leaf, arch)
    gl = torch.autograd.grad(loss, [leaf[k] for k in names], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaf[k])) for k, g in zip(names, gl)}
    return dict(loss=loss.detach(), probs=probs.detach(), grads=grads, state=state)
