"""Host-side helpers of the class-imbalance losses (LOSS.* of the config, X3D.set_loss): class weights from the class counts
of a training set.  NumPy only; the weights themselves act on the device (x3d_softmax_xent_w / x3d_sigmoid_bce_w)."""
import numpy as np

SCHEMES = ("inverse", "effective")


def class_weights_from_counts(counts, scheme: str = "inverse", beta: float = 0.999):
    """Per-class loss weights [classes] float64 from the number of training samples per class.
      "inverse":   w_c = 1 / n_c
      "effective": w_c = (1 - beta) / (1 - beta ** n_c), the inverse effective number of samples (Cui et al., Class-Balanced
                   Loss Based on Effective Number of Samples, CVPR 2019); beta in [0, 1): 0 weighs every class alike, beta -> 1
                   approaches "inverse".
    Either way the weights are normalised to mean 1 over the classes with a non-zero count, so the loss keeps its scale; a
    class without samples gets weight 0 (it never occurs as a label, and under mixup / in the sigmoid head it adds nothing).
    ValueError for a count that is negative or not finite, no class with a sample, an unknown scheme or a beta outside [0, 1)."""
    n = np.asarray(counts, dtype=np.float64)
    if n.ndim != 1 or n.size == 0:
        raise ValueError(f"counts must be a non-empty vector, got shape {n.shape}")
    if not np.all(np.isfinite(n)) or np.any(n < 0):
        raise ValueError("counts must be finite and >= 0")
    have = n > 0
    if not have.any():
        raise ValueError("every class count is zero")
    if scheme not in SCHEMES:
        raise ValueError(f"scheme must be one of {SCHEMES}, not {scheme!r}")
    w = np.zeros_like(n)
    if scheme == "inverse":
        w[have] = 1.0 / n[have]
    else:
        beta = float(beta)
        if not 0.0 <= beta < 1.0:
            raise ValueError(f"beta must lie in [0, 1), not {beta}")
        # 1 - beta^n = -expm1(n log beta): no cancellation for beta close to 1 (beta = 0: log = -inf, expm1 = -1)
        with np.errstate(divide="ignore"):
            w[have] = (1.0 - beta) / -np.expm1(n[have] * np.log(beta))
    w[have] *= have.sum() / w[have].sum()
    return w
