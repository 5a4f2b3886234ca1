"""
TEST-ONLY reference of the atom terms, gains and Gram under a beta-divergence (include/tnmf_hip.h, "atom terms, beta"):
independent of the host fallback (tnmf_amd.atoms_host.atom_divergence_terms_numpy), which shares neither its parts nor its
forms.  The parts R_m come from tests/atoms_reference.py (``parts_valid`` / ``parts_loop``); the element divergence is that of
tests/beta_reference.py::divergence, written per element.

The gain is the definition taken literally, D(V | x_m) - D(V | x), with the two divergences evaluated in extended precision
(numpy's longdouble: 64 bits of mantissa where the tests run) so that the subtraction loses nothing that a float64 result
could show; ``a``, ``b`` and ``B`` are sums of products of float64 factors.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2. ** -63, 'the reference of the gain needs an extended-precision longdouble'


def element(V, x, beta):
    """d_beta(V | x) per element, x > 0 (clamped and shifted by eps already), in the dtype of the operands."""
    if beta == 1:
        with np.errstate(divide='ignore', invalid='ignore'):
            vlog = np.where(V > 0, V * np.log(np.where(V > 0, V, 1) / x), 0)
        return vlog - V + x
    if beta == 0:
        q = V / x
        return q - np.log(q) - 1
    return (V ** beta + (beta - 1) * x ** beta - beta * V * x ** (beta - 1)) / (beta * (beta - 1))


def weights(V, G):
    """G clipped at 0 (ones without weights), and V with zeros where the weight is <= 0: what V holds there is not data."""
    g = np.ones(np.shape(V)) if G is None else np.where(np.asarray(G, dtype=np.float64) > 0, G, 0.)
    with np.errstate(invalid='ignore'):
        return g, np.where(g > 0, np.asarray(V, dtype=np.float64), 0.)


def factors(V, R, G, beta, eps):
    """(gd, gw) = (G (V x^(beta-2) - x^(beta-1)), G c), c = (beta-1) x^(beta-2) + (2-beta) V x^(beta-3), x = max(R, 0) +
    eps; exact zeros where the weight is <= 0.  Each from the factored form, whose one difference is of the operands."""
    g, v = weights(V, G)
    x = np.maximum(np.asarray(R, dtype=np.float64), 0.) + eps
    gd = g * (v - x) * x ** (beta - 2.)
    gw = g * ((beta - 1.) * x + (2. - beta) * v) * x ** (beta - 3.)
    return np.where(g > 0, gd, 0.), np.where(g > 0, gw, 0.)


def factors_abs(V, R, G, beta, eps):
    """The same two factors with every term taken by its absolute value, G (V + x) x^(beta-2) and G (|beta-1| x +
    |2-beta| V) x^(beta-3): the size an error of x -- a reconstruction the library computed itself -- is measured against
    (a relative error e of x moves gd by at most (|beta-2| + 1) e and gw by at most (|beta-3| + 1) e times these)."""
    g, v = weights(V, G)
    x = np.maximum(np.asarray(R, dtype=np.float64), 0.) + eps
    return g * (v + x) * x ** (beta - 2.), g * (abs(beta - 1.) * x + abs(2. - beta) * v) * x ** (beta - 3.)


def curvature_is_negative(V, R, G, beta, eps):
    """(pixels with weight > 0 and c < 0, pixels with weight > 0)"""
    g, _ = weights(V, G)
    _, gw = factors(V, R, G, beta, eps)
    return int(np.sum((g > 0) & (gw < 0))), int(np.sum(g > 0))


def gain_terms(parts, V, G, R, beta, eps):
    """G (d_beta(V | x_m) - d_beta(V | x)) per (sample, atom, channel, pixel), float64, x_m = max(R - R_m, 0) + eps: the
    two divergences and their difference in extended precision.  Exact zeros where R_m == 0 or the weight is <= 0."""
    g, v = weights(V, G)
    R = np.asarray(R, dtype=np.float64)
    x = (np.maximum(R, 0.).astype(LD) + LD(eps))[:, None]
    xm = np.maximum(R.astype(LD)[:, None] - parts.astype(LD), 0) + LD(eps)
    vl = v.astype(LD)[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):   # (entries of weight <= 0 hold V = 0: dropped below)
        diff = element(vl, xm, LD(beta)) - element(vl, x, LD(beta))
    live = (g[:, None] > 0) & (parts != 0)
    return np.where(live, g.astype(LD)[:, None] * diff, 0).astype(np.float64)


def terms(parts, V, G, R, beta, eps):
    """dict(a, b, gain [N, Mo], scale_a = sum R_m |gd|, scale_b = sum |gw| R_m^2, scale_gain = sum |gain terms|)"""
    R = parts.sum(axis=1) if R is None else R
    gd, gw = factors(V, R, G, beta, eps)
    axes = tuple(range(2, parts.ndim))
    t = gain_terms(parts, V, G, R, beta, eps)
    return dict(a=np.sum(parts * gd[:, None], axis=axes), b=np.sum(gw[:, None] * parts ** 2, axis=axes),
                gain=np.sum(t.astype(LD), axis=axes).astype(np.float64),
                scale_a=np.sum(np.abs(parts) * np.abs(gd[:, None]), axis=axes),
                scale_b=np.sum(np.abs(gw[:, None]) * parts ** 2, axis=axes), scale_gain=np.sum(np.abs(t), axis=axes))


def gain_bound(parts, V, G, R, beta, eps, n, u):
    """(n + 8) u sum G R_m max(|f(x_lo)|, |f(x_hi)|) with f(x) = x^(beta-1) - V x^(beta-2), the derivative of d_beta(V | x)
    in x, at x_lo/hi = max(R - R_m -/+ (n + 2) u R_m, 0) + eps: the rounding of R_m, a chain of n products in the element
    type, moved through the divergence, and the epilogue's own roundings in double."""
    g, v = weights(V, G)
    R = np.asarray(R, dtype=np.float64)[:, None]
    v = v[:, None]
    worst = np.zeros(parts.shape)
    for sign in (-1., 1.):
        x = np.maximum(R - parts + sign * (n + 2) * u * parts, 0.) + eps
        worst = np.maximum(worst, np.abs(x ** (beta - 1.) - v * x ** (beta - 2.)))
    return (n + 8) * u * np.sum(g[:, None] * np.abs(parts) * worst, axis=tuple(range(2, parts.ndim)))


def gram(parts, V, G, R, beta, eps):
    """(B, scale_B): B[n, m, m'] = sum G c R_m R_m' and the same sum over |G c|."""
    R = parts.sum(axis=1) if R is None else R
    _, gw = factors(V, R, G, beta, eps)
    N, Mo = parts.shape[:2]
    flat, w = parts.reshape(N, Mo, -1), gw.reshape(N, 1, -1)
    return np.einsum('nmx,nkx->nmk', flat * w, flat), np.einsum('nmx,nkx->nmk', flat * np.abs(w), flat)
