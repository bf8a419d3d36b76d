"""Host restatements for the device loss scaler (SOLVER.DEVICE_LOSS_SCALE): Keras' DynamicLossScale as `Trainer._update` applies
it on the host, on the eight-slot state x3d_loss_scale_update keeps (include/x3d_hip.h), and the fp64 Adam step the
bias-correction test compares with.  Plain Python and numpy: no device, no package import."""
import numpy as np

SCALE, INV, GOOD, SKIPPED, APPLIED, LAST_SKIPPED = range(6)
STATE = 8


def initial(scale=2.0 ** 15, applied=0, skipped=0):
    return [float(scale), 1.0 / float(scale), 0.0, float(skipped), float(applied), 0.0, 0.0, 0.0]


def float32_finite(x) -> bool:
    with np.errstate(over="ignore"):
        return bool(np.isfinite(np.float32(x)))


def update(state, nonfinite: bool, growth_steps: int):
    """One update of the rule.  nonfinite: the gradient held an inf / nan (norm[1] != 0) -- the step is skipped, the scale
    halved down to 1 at the least and the run of finite steps ends.  Else the step counts as applied and as one more finite
    step in a row; after `growth_steps` of them the scale doubles (if twice the scale is still a finite float32) and the run
    starts again.  Returns the new state; slot INV stays 1 / scale."""
    if growth_steps < 1:
        raise ValueError("growth_steps counts from 1")
    s = list(state)
    if nonfinite:
        s[SCALE] = max(s[SCALE] / 2.0, 1.0)
        s[GOOD] = 0.0
        s[SKIPPED] += 1.0
        s[LAST_SKIPPED] = 1.0
    else:
        s[APPLIED] += 1.0
        s[GOOD] += 1.0
        s[LAST_SKIPPED] = 0.0
        if s[GOOD] >= growth_steps and float32_finite(2.0 * s[SCALE]):
            s[SCALE] *= 2.0
            s[GOOD] = 0.0
    s[INV] = 1.0 / s[SCALE]
    return s


def run(state, script, growth_steps):
    """the states after each entry of `script` (an iterable of nonfinite flags)"""
    out = []
    for bad in script:
        state = update(state, bool(bad), growth_steps)
        out.append(state)
    return out


def adam_step(w, m, v, g, l2, lr, step, wd, beta1=0.9, beta2=0.999, eps=1e-7, c=1.0):
    """tf.optimizers.Adam + the coupled L2 term in fp64 (numpy arrays; l2: 0 / 1 mask): g' = c g + 2 wd w where l2, the moments,
    and w -= lr_t m / (sqrt(v) + eps) with lr_t = lr sqrt(1 - beta2^step) / (1 - beta1^step).  Returns (w, m, v)."""
    w, m, v, g = (np.asarray(a, dtype=np.float64) for a in (w, m, v, g))
    gi = c * g + 2.0 * wd * w * np.asarray(l2, dtype=np.float64)
    m = beta1 * m + (1.0 - beta1) * gi
    v = beta2 * v + (1.0 - beta2) * gi * gi
    lr_t = lr * np.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
    return w - lr_t * m / (np.sqrt(v) + eps), m, v
