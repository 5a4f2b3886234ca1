"""
TEST-ONLY reference of the W side of the events (include/tnmf_hip.h, "events", tnmf_hip_events_grad_W): float64, written
straight from the image table over ``events_reference.pixels`` and on purpose naive -- one Python loop per event, per image
and per pixel.  Independent of the front end's host fallback (tnmf_amd.TransformInvariantNMF.events_fit_numpy), which clips
slices per image.
"""
import numpy as np

import events_reference as eref
from tnmf_amd import transforms as tr


def grad_W(V, R, W, D, mode, sample, plane, shift, strength):
    """[2, P, C, *A] in float64: neg (against V) and pos (against R) of the events, duplicates added up.  ``pixels`` walks a
    dictionary that holds the flat index of each entry, so every pixel comes with the entry of W it belongs to."""
    V, R = np.asarray(V, dtype=np.float64), np.asarray(R, dtype=np.float64)
    taps = np.arange(W.size, dtype=np.float64).reshape(W.shape)
    out = np.zeros((2, W.size))
    for n, p, u, h in zip(sample, plane, np.asarray(shift).reshape(len(sample), -1), strength):
        for at, tap in eref.pixels(taps, D, mode, n, p, u):
            out[0, int(tap)] += float(h) * V[at]
            out[1, int(tap)] += float(h) * R[at]
    return out.reshape((2,) + W.shape)


def step_W(V, W, mode, sample, plane, shift, strength, eps=1e-9, transforms=None):
    """W after one multiplicative W step on the events: the gradient of the (expanded) dictionary, folded, MU, each atom
    normalised to sum 1 over its shift axes per channel; an atom whose neg is zero in every entry keeps its entries."""
    D, N = V.shape[2:], V.shape[0]
    W_eff = W if transforms is None else tr.expand(W, transforms)
    R = eref.render(W_eff, D, N, mode, sample, plane, shift, strength)
    neg, pos = grad_W(V, R, W_eff, D, mode, sample, plane, shift, strength)
    if transforms is not None:
        neg, pos = tr.fold(neg, transforms), tr.fold(pos, transforms)
    new = np.array(W, dtype=np.float64)
    for m in range(len(W)):
        if neg[m].any():
            new[m] = W[m] * neg[m] / (pos[m] + eps)
            new[m] /= new[m].sum(axis=tuple(range(1, new[m].ndim)), keepdims=True)
    return new


def fit(V, W, mode, sample, plane, shift, strength, n_iterations, sparsity=0., eps=1e-9, update_H=True, update_W=True,
        transforms=None):
    """(W, strengths) after n_iterations of: one ``events_reference.refit`` step of the strengths, one W step."""
    W, h = np.array(W, dtype=np.float64), np.array(strength, dtype=np.float64)
    for _ in range(n_iterations):
        if update_H:
            W_eff = W if transforms is None else tr.expand(W, transforms)
            h = eref.refit(V, W_eff, mode, sample, plane, shift, h, 1, sparsity, eps)
        if update_W:
            W = step_W(V, W, mode, sample, plane, shift, h, eps, transforms)
    return W, h
