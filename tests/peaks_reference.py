"""
TEST-ONLY reference of the detections (include/tnmf_hip.h, "detections"): brute force, written straight from the
definition and on purpose naive -- every candidate is compared with EVERY entry of its sample and suppression group,
coordinate by coordinate.  Independent of the front end's host fallback (tnmf_amd.TransformInvariantNMF.find_peaks_numpy),
which cuts one window per candidate.
"""
import numpy as np


def find_peaks(H, threshold, radius, group=1):
    """(idx, val): ascending flat C-order indices in H[N, P, *S] of the detections, and H's entries there.

    x = (n, p, u) is a detection iff H[x] > threshold and no y = (n, q, v) != x with q in the run of `group` planes that
    holds p and |v_k - u_k| <= radius[k] for every k has H[y] > H[x], or H[y] == H[x] and a lower flat index."""
    H = np.asarray(H)
    N, P, S = H.shape[0], H.shape[1], H.shape[2:]
    assert len(radius) == len(S) and group >= 1 and P % group == 0
    flat_of = np.arange(H.size, dtype=np.int64).reshape(H.shape)
    found = []
    for n in range(N):
        for g0 in range(0, P, group):
            block = H[n, g0:g0 + group].astype(np.float64).reshape(-1)          # (float32 -> float64 is exact)
            flat = flat_of[n, g0:g0 + group].reshape(-1)
            coords = np.stack(np.unravel_index(np.arange(block.size), (group,) + tuple(S)), axis=1)[:, 1:]
            cand = np.flatnonzero(block > float(threshold))
            for lo in range(0, len(cand), 256):                                   # (chunks bound the pairwise tables)
                c = cand[lo:lo + 256]
                near = np.ones((len(c), block.size), dtype=bool)
                for k, r in enumerate(radius):
                    near &= np.abs(coords[c, k][:, None] - coords[None, :, k]) <= r
                other = flat[c][:, None] != flat[None, :]
                hx, hy = block[c][:, None], block[None, :]
                stronger = (hy > hx) | ((hy == hx) & (flat[None, :] < flat[c][:, None]))
                suppressed = np.any(near & other & stronger, axis=1)
                found.append(flat[c[~suppressed]])
    idx = np.sort(np.concatenate(found)) if found else np.zeros(0, dtype=np.int64)
    return idx, H.reshape(-1)[idx]


def detections(H_property, threshold, radius, group, atom_shape, mode, n_transforms=1, max_per_sample=None):
    """The rows ``TransformInvariantNMF.detections`` must return for a model whose ``H`` property is ``H_property``
    ([N, M, *S] or with transforms [N, M, T, *S]): dict of sample, atom, transform, shift, origin, strength."""
    H = np.asarray(H_property)
    k = len(atom_shape)
    Hp = H.reshape((H.shape[0], -1) + H.shape[-k:])
    idx, val = find_peaks(Hp, threshold, radius, group)
    at = np.unravel_index(idx, Hp.shape)
    rows = list(range(len(idx)))
    if max_per_sample is not None:
        rows = []
        for n in np.unique(at[0]):
            mine = [i for i in range(len(idx)) if at[0][i] == n]
            mine.sort(key=lambda i: (-float(val[i]), idx[i]))
            rows += mine[:max_per_sample]
        rows.sort()
    rows = np.asarray(rows, dtype=np.int64)
    shift = np.stack([a[rows] for a in at[2:]], axis=1).reshape(len(rows), k)
    off = np.array([a - 1 if mode == 'valid' else 0 for a in atom_shape])
    return dict(sample=at[0][rows], atom=at[1][rows] // n_transforms, transform=at[1][rows] % n_transforms,
                shift=shift, origin=shift - off, strength=val[rows])


def assert_equal(det, want):
    """`det` (a Detections record) equals the dict `want`, exactly: index arrays equal, strengths bit for bit."""
    for name in ('sample', 'atom', 'transform', 'shift', 'origin'):
        np.testing.assert_array_equal(getattr(det, name), want[name], err_msg=name)
    assert det.strength.dtype == want['strength'].dtype
    assert det.strength.tobytes() == want['strength'].tobytes()
