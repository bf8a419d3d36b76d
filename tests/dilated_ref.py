"""The dilated channelwise conv of NETWORK.RES5_DILATION restated on the CPU (include/x3d_hip.h K6, dilated form):
Conv3D(k = 3x3x3, strides 1, dilation (1, d, d), groups = C), padding 1 in time and d on each spatial side, so the output has
the input's extents.  fp64 stencils of the forward and the fused backward for the kernel parity tests, and the oracle's
Storage with the dilation applied at the sites of the last stage for the model-level ones (oracle/ itself is unchanged:
res_block routes the conv through Storage.depthwise)."""
import torch
import torch.nn.functional as F

from oracle import x3d_oracle as O


def dilated3x3x3(x, w, d):
    """x [N][C][T][H][W], w [C][3][3][3] -> [N][C][T][H][W]; d = 1 is the dense stride-1 conv (TF-SAME is symmetric there)."""
    c = x.shape[1]
    return F.conv3d(x, w.reshape(c, 1, 3, 3, 3), padding=(1, d, d), dilation=(1, d, d), groups=c)


def _affine(x, ss):
    return x * ss[:, 0].view(1, -1, 1, 1, 1) + ss[:, 1].view(1, -1, 1, 1, 1)


def fwd_ref(x, w, d, ss=None, act=0):
    """y = conv(act(s * x + t)) in fp64; ss [C][2] or None, act 0 none / 1 relu.  The padding is zeros AFTER the prologue."""
    u = x.double() if ss is None else _affine(x.double(), ss.double())
    if act == 1:
        u = F.relu(u)
    return dilated3x3x3(u, w.double(), d)


def bwd_ref(dv, braw, coef_nc, araw, ss_a, w, d):
    """The fused backward in fp64: dB = A dv + B braw + C per (n, c); ga = (conv^T dB) [s_a araw + t_a > 0];
    dw [C][27] = sum dB * relu(s_a araw + t_a) over the taps.  Returns (ga, dw)."""
    cd = coef_nc.double()
    dB = cd[:, :, 0, None, None, None] * dv.double() + cd[:, :, 1, None, None, None] * braw.double() + cd[:, :, 2, None, None, None]
    z = _affine(araw.double(), ss_a.double())
    act = F.relu(z).requires_grad_(True)
    wref = w.double().clone().requires_grad_(True)
    dA, dW = torch.autograd.grad((dilated3x3x3(act, wref, d) * dB).sum(), [act, wref])
    return dA * (z > 0), dW.reshape(-1, 27)


class DilatedStorage(O.Storage):
    """oracle Storage whose depthwise() is dilated at `sites` ({block prefix: d}); every other site is the oracle's own.  The
    dilated kernels multiply fp32 operands in every storage type (no matrix-core form), so those sites never round theirs."""

    def __init__(self, dtype=None, dw_operands=None, sites=None):
        super().__init__(dtype, dw_operands)
        self.sites = dict(sites or {})

    def depthwise(self, a_act, w, stride, site):
        d = self.sites.get(site, 1)
        if d == 1:
            return super().depthwise(a_act, w, stride, site)
        assert stride == 1, f"{site}: a dilated conv at stride {stride}"
        return dilated3x3x3(a_act, w, d)


def dilated_sites(arch):
    """{block prefix: dilation} of the blocks whose `b` conv is dilated"""
    return {O.block_prefix(b): b.dilation for b in arch.blocks if b.dilation > 1}
