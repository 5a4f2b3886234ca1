"""
The contract of tnmf_hip_run_schedule (include/tnmf_hip.h) in float64: a plain NumPy interpreter of an operation list on
the oracle's primitives (oracle/tnmf_oracle.py: gradient_H, gradient_W, normalize).  The list is executed as written --
nothing is joined, nothing is fused -- on one, two or three shift axes:

  ('H', s)         H[s] *= neg / (pos + eps + sparsity)                  (TransformInvariantNMF.py:227-230)
  ('G', s, a, b)   acc = b * g when a == 0, WHATEVER acc held (NaN included); else acc = a * acc + b * g; g = [neg | pos]
                   of the W gradient on the samples s, zero for an empty slice
  ('W',)           acc_pos += eps AND STAYS incremented (:232); W = W * acc_neg / acc_pos; W normalised over the atom axes

Besides (W, H, acc) it returns, per output, the length of the longest chain of dependent half steps behind it, counted
from the list: an H half step (reconstruct + correlation with W) is one link, a W gradient (reconstruct + correlation with
H) is one link -- the W half step it belongs to adds none of its own, ('W',) is an elementwise quotient and a row sum --
and a link stands on the longest chain among what it reads.  The bars of tests/test_hip_schedule_matrix.py are the
project's bar of one fused half step times that length.
"""
import numpy as np

from oracle import tnmf_oracle as orc


def as_slice(s, N):
    lo, hi, step = s.indices(N)
    assert step == 1
    return slice(lo, max(lo, hi))


def chains(ops, N):
    """{'W': , 'H': , 'acc': } -- the longest chain of dependent half steps behind each output of the list (0: untouched
    or exact), and 'H_per_sample'."""
    dW, dacc, dH = 0, 0, np.zeros(N, dtype=int)
    for op in ops:
        if op[0] == 'H':
            s = as_slice(op[1], N)
            dH[s] = np.maximum(dH[s], dW) + 1
        elif op[0] == 'G':
            s = as_slice(op[1], N)
            dg = (max(dW, int(dH[s].max())) + 1) if s.stop > s.start else 0
            dacc = dg if op[2] == 0 else max(dacc, dg)
        elif op[0] == 'W':
            dW = max(dW, dacc)
        else:
            raise ValueError(op)
    return {'W': int(dW), 'H': int(dH.max()) if N else 0, 'acc': int(dacc), 'H_per_sample': dH}


def run(V, W, H, acc, ops, eps=1e-9, sparsity=0.):
    """-> (W, H, acc, chains): the list on copies of the float64 operands."""
    V = np.asarray(V, dtype=np.float64)
    W, H, acc = (np.array(x, dtype=np.float64) for x in (W, H, acc))
    k = W.ndim - 2
    impl = 'c' if k < 3 else 'contract'
    axes = tuple(range(-k, 0))
    N = H.shape[0]
    assert acc.shape == (2,) + W.shape
    for op in ops:
        if op[0] == 'H':
            s = as_slice(op[1], N)
            if s.stop > s.start:
                neg, pos = orc.gradient_H(V, W, H, s, impl)
                H[s] *= neg / (pos + eps + (sparsity if sparsity > 0 else 0.))
        elif op[0] == 'G':
            s, a, b = as_slice(op[1], N), op[2], op[3]
            g = np.stack(orc.gradient_W(V, W, H, s, impl)) if s.stop > s.start else np.zeros_like(acc)
            acc = b * g if a == 0 else a * acc + b * g
        elif op[0] == 'W':
            acc[1] += eps
            W = W * acc[0] / acc[1]
            orc.normalize(W, axes)
        else:
            raise ValueError(op)
    return W, H, acc, chains(ops, N)
