"""
TEST-ONLY reference of the per-source signals (include/tnmf_hip.h, "sources"): float64, built on
``atoms_reference.parts_valid`` -- one correlation per plane of the PADDED activations -- and independent of the front
end's host fallback (tnmf_amd.sources_host).
"""
import numpy as np

import atoms_reference as aref


def source_sums(W, Hp, plane_sets):
    """(r [N, S, C, *D], total [N, C, *D]): per source the sum of its planes' parts (``plane_sets``: S lists of planes), and
    the sum over every plane, listed or not."""
    parts = aref.parts_valid(W, Hp, 1)
    r = np.stack([parts[:, list(planes)].sum(axis=1) for planes in plane_sets], axis=1)
    return r, parts.sum(axis=1)


def outputs(W, Hp, V, plane_sets, eps):
    """dict(contribution, mask, masked [N, S, C, *D]; label, share [N, *D]; total [N, C, *D]); 0 where total + eps is 0."""
    r, total = source_sums(W, Hp, plane_sets)
    den = (total + eps)[:, None]
    mask = np.divide(r, den, out=np.zeros(r.shape), where=den != 0)
    rc, tc = r.sum(axis=2), total.sum(axis=1)
    label = np.full(tc.shape, -1, dtype=np.int32)
    best = np.zeros(tc.shape)
    for g in range(rc.shape[1]):   # the first source starts, then strict >: the lowest index wins a tie
        better = rc[:, g] > best if g else np.ones(tc.shape, dtype=bool)
        label[better], best[better] = g, rc[:, g][better]
    label[tc == 0] = -1
    share = np.divide(best, tc + eps, out=np.zeros(tc.shape), where=tc + eps != 0)
    return dict(contribution=r, mask=mask, masked=np.asarray(V, dtype=np.float64)[:, None] * mask, label=label,
                share=share, total=total)
