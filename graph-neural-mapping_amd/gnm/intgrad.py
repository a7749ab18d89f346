"""Quadrature rules of GIN_InfoMaxReg.integrated_gradients(): the path integral over alpha in [0, 1] of the input
gradient at x' + alpha (X - x') as sum_k w_k grad(alpha_k).  Host arithmetic in fp64; the driver
(gnm/core.py integrated_gradients_hip) casts the two arrays once to fp32 for the device."""
import numpy as np

METHODS = ("midpoint", "trapezoid", "gausslegendre")


def quadrature(method, steps):
    """(alphas, weights): two float64 arrays of `steps` nodes in [0, 1] and their weights (which sum to 1).
    "midpoint": alpha_k = (k + 1/2) / K, w_k = 1 / K.  "trapezoid": alpha_k = k / (K - 1), endpoints included with
    half weight, K >= 2.  "gausslegendre": numpy.polynomial.legendre.leggauss(K) mapped from [-1, 1] to [0, 1], exact
    for polynomials of degree 2 K - 1.  ValueError for an unknown method or too few steps."""
    if method not in METHODS:
        raise ValueError("integrated_gradients: method must be one of %s, not %r" % (METHODS, method))
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)):
        raise ValueError("integrated_gradients: steps must be an integer, not %r" % (steps,))
    K = int(steps)
    least = 2 if method == "trapezoid" else 1
    if K < least:
        raise ValueError("integrated_gradients: method %r needs steps >= %d, got %d" % (method, least, K))
    if method == "midpoint":
        return (np.arange(K, dtype=np.float64) + 0.5) / K, np.full(K, 1.0 / K)
    if method == "trapezoid":
        w = np.full(K, 1.0 / (K - 1))
        w[0] = w[-1] = 0.5 / (K - 1)
        return np.arange(K, dtype=np.float64) / (K - 1), w
    x, w = np.polynomial.legendre.leggauss(K)
    return 0.5 * (x + 1.0), 0.5 * w
