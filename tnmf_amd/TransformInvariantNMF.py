"""
Front end of the MI355X shift-invariant NMF: the multiplicative-update schedules that drive a backend.

Public surface = the reference's (tnmf/TransformInvariantNMF.py): ``TransformInvariantNMF(n_atoms, atom_shape,
inhibition_range, backend, logger, verbose, **backend_kwargs)`` with ``fit`` / ``fit_batch`` / ``fit_minibatches`` /
``fit_stream``, the read-outs ``W``, ``H``, ``V``, ``R``, ``R_partial(i)`` and the ``MiniBatchAlgorithm`` enum; beyond it
``detections()`` (-> ``Detections``), the events read off ``H``, and ``reconstruct_detections`` / ``refit_detections``,
what such a list explains and its strengths refitted on the fixed support, and ``detection_gains`` / ``prune_detections``,
what each row explains and the list without the rows the data does not need, and ``pursue_detections``, the list found by
forward selection, without a dense fit of H.
The only backend shipped is ``'hip'`` (tnmf_amd/backends/HIP.py); any object implementing
tnmf_amd.backends._Backend.Backend can be passed instead of a name.

Differences from the reference, all deliberate:
  * when the backend offers the fused hooks (``fused_update_H`` / ``fused_update_W`` / ``multiplicative_update``)
    they replace the three elementwise passes of TransformInvariantNMF.py:232-235 -- same arithmetic, less traffic;
    ``use_fused_updates=False`` restores the call-by-call form of the reference;
  * the per-iteration energy is evaluated only if the logger is enabled for INFO (the reference formats it eagerly,
    TransformInvariantNMF.py:346, which costs a reconstruction per iteration).
"""
import dataclasses
import enum
import itertools
import logging
import math
import warnings
from typing import Callable, Iterable, Iterator, List, Optional, Tuple, Union

import numpy as np

from . import _args
from . import transforms as _transforms
from .atoms_host import (atom_divergence_gram_numpy, atom_divergence_terms_numpy, atom_gram_numpy, atom_terms_numpy,
                         gram_drop, gram_elimination, gram_scales, gram_set_gain, pad_activations_numpy)
from .backends._Backend import Backend, sliceNone
from .correlogram_host import activation_correlogram_numpy, cooccurrence
# (the host side of the events; the names stay importable from this module)
from .events_host import (event_boxes, event_images, events_alternatives_numpy, events_fit_numpy,  # noqa: F401
                          events_gain_numpy, events_gram_numpy, events_inverse_diag_numpy, events_landscape_numpy,
                          events_norms_numpy, events_numpy, events_solve_numpy, find_peaks_numpy, landscape_gains, pursuit_loop, pursuit_numpy,
                          relabel_hops, relocation_hops)
from .patches_host import (FRAMES as _PATCH_FRAMES, SOURCES as _PATCH_SOURCES, event_patch_moments_numpy,  # noqa: F401
                           event_patches_numpy, modes_from_moments)
from .sources_host import OUTPUTS as _SOURCE_OUTPUTS, dominant_numpy, separate_numpy, source_tables
from .triggered_host import extend_atoms, tap_gains_from_sums, triggered_sums_numpy, window_gains

# the fields activation_triggered_sums correlates the activations with
_TRIGGERED_SOURCES = ('data', 'reconstruction', 'residual')


class MiniBatchAlgorithm(enum.Enum):
    """Mini-batch MU schedules of Serizel et al. 2016 (reference: TransformInvariantNMF.py:47-55)."""
    Cyclic_MU = 4
    ASG_MU = 5
    GSG_MU = 6
    ASAG_MU = 7
    GSAG_MU = 8


def _sequential_minibatches(length: int, batch_size: Optional[int]) -> List[slice]:
    if batch_size is None:
        return [sliceNone]
    return [slice(lo, min(lo + batch_size, length)) for lo in range(0, length, batch_size)]


def _permuted(items: list) -> list:
    # one np.random.permutation call per epoch, like the reference's _random_shuffle (:40-44)
    order = np.random.permutation(len(items))
    return [items[i] for i in order]


def _joined(batches: list) -> list:
    """A run of H half steps on pairwise disjoint sample slices commutes (the H update of a sample reads that sample and W
    only, reference :246-271, and W does not change inside the run): the slices sorted and joined where they touch.
    Overlapping or strided slices: the list as it is."""
    spans = []
    for b in batches:
        lo, hi = b.start, b.stop
        if b.step not in (None, 1) or lo is None or hi is None or lo < 0 or hi < 0:
            return list(batches)
        if hi > lo:
            spans.append((lo, hi))
    spans.sort()
    if any(spans[i][0] < spans[i - 1][1] for i in range(1, len(spans))):
        return list(batches)
    out = []
    for lo, hi in spans:
        if out and out[-1][1] == lo:
            out[-1][1] = hi
        else:
            out.append([lo, hi])
    return [slice(lo, hi) for lo, hi in out]


_BETA_NAMES = {'frobenius': 2., 'kullback-leibler': 1., 'itakura-saito': 0.}


def beta_loss_value(beta_loss) -> float:
    """beta of ``beta_loss``: scikit-learn's names ('frobenius' 2, 'kullback-leibler' 1, 'itakura-saito' 0) or a finite
    number; anything else raises ValueError."""
    if isinstance(beta_loss, str):
        if beta_loss not in _BETA_NAMES:
            raise ValueError(f'beta_loss must be one of {sorted(_BETA_NAMES)} or a finite float, not {beta_loss!r}')
        return _BETA_NAMES[beta_loss]
    if _args.is_bool(beta_loss) or not isinstance(beta_loss, (int, float, np.integer, np.floating)):
        raise ValueError(f'beta_loss must be one of {sorted(_BETA_NAMES)} or a finite float, not {beta_loss!r}')
    beta = float(beta_loss)
    if not np.isfinite(beta):
        raise ValueError(f'beta_loss must be finite, not {beta_loss!r}')
    return beta


def _backend_registry():
    from .backends.HIP import HIP_Backend
    return {'hip': HIP_Backend}


ProgressCallback = Callable[['TransformInvariantNMF', int], bool]


@dataclasses.dataclass(frozen=True)
class Detections:
    """The detections of a fitted model (``TransformInvariantNMF.detections``): K rows in the C order of the ``H`` property.

    sample    [K] index of the sample in the order of ``V`` (with a process group: this rank's samples, offset by the start
              of its shard)
    atom      [K] atom m
    transform [K] orientation t of the atom (0 without transforms)
    shift     [K, k] index into the k shift axes of ``H``
    origin    [K, k] sample coordinate of the atom's first pixel: the occurrence covers ``origin .. origin + atom_shape - 1``
              (``shift - (atom_shape - 1)`` in 'valid' mode, ``shift`` in 'full' / 'circular' / 'reflect'); positions outside
              the sample belong to a partly visible, wrapped or mirrored occurrence
    strength  [K] the entries of ``H``, bit for bit
    """
    sample: np.ndarray
    atom: np.ndarray
    transform: np.ndarray
    shift: np.ndarray
    origin: np.ndarray
    strength: np.ndarray

    def __len__(self) -> int:
        return len(self.sample)


class TransformInvariantNMF:
    r"""
    Shift-invariant non-negative matrix factorisation ``V ~ sum_m H[:, m] (*) W[m]`` by multiplicative updates.

    Parameters
    ----------
    n_atoms, atom_shape : dictionary size; ``W`` has shape ``(n_atoms, n_channels, *atom_shape)``
    inhibition_range : lateral inhibition range per shift axis (default ``atom_shape - 1``)
    backend : ``'hip'`` or a :class:`~tnmf_amd.backends._Backend.Backend` instance
    logger, verbose : as in the reference (0 errors .. 3 debug)
    use_fused_updates : use the backend's fused half-step kernels when no inhibition term is requested
    beta_loss : the objective, D_beta(V | R): ``'frobenius'`` / 2 (default, 1/2 ||V - R||^2), ``'kullback-leibler'`` / 1,
                ``'itakura-saito'`` / 0 or any finite float (scikit-learn's names).  beta != 2 runs the multiplicative
                updates of Serizel et al. 2016 on the backend's beta hooks, step by step (no one-call schedules), and the
                energy reports D_beta of R + eps; it needs V > 0 for beta <= 0.
    ``fit`` / ``fit_batch`` / ``fit_minibatches`` take ``weights``: a finite, non-negative array that broadcasts to V's shape
    (e.g. ``[N, 1, *D]`` a pixel mask shared by the channels, ``[N, 1, 1, 1]`` per-sample weights), for the weighted
    objective sum G * D_beta(V | R).  Entries of V whose weight is 0 are not data and may hold anything.  A weighted fit
    runs on the backend's hooks step by step, like beta != 2; each fit stands alone (a later fit without weights is
    unweighted).  Not for volumes, not for ``fit_stream``.
    transforms : ``None`` (default: shifts only), or a group of atom transforms the model is invariant to as well --
                 ``'flip'`` (T = 2: the atom and its mirror along the last axis; 1 or 2 shift axes), ``'mirrors'`` (T = 4:
                 the mirrors along x, y and both), ``'rot90'`` (T = 4: rotations by k * 90 degrees, ``np.rot90(a, k)``;
                 square atoms) or ``'dihedral'`` (T = 8: the rotations, then the rotations of the mirror along x; square
                 atoms); tnmf_amd/transforms.py.  Each of the ``n_atoms`` atoms then stands for T effective atoms
                 ``T_t(W[m])``: ``W`` stays ``[M, C, *A]``, ``H`` is ``[N, M, T, *shift]``, ``transformed_atoms`` is
                 ``[M, T, C, *A]``.  The effective atoms are atoms for everything on the H side (sparsity, lateral and
                 cross-atom inhibition over all M * T of them); the W step folds their gradient back onto W.  A transformed
                 fit runs on the backend's hooks step by step, like beta != 2.  Not for volumes.
                 Or an ``AtomOperators`` on atoms of ``atom_shape`` (tnmf_amd/transforms.py: ``rotations(A, n)`` by any
                 angle, ``scales(A, factors)``, ``compose(outer, inner)``, ``from_dense(L)``, ``from_group(name, A)``):
                 T non-negative linear maps ``L_t``, ``W_eff[m * T + t, c] = L_t W[m, c]``, everything above with
                 T = ``ops.T`` and the W gradient folded with the transposes; the backend must declare
                 ``supports_atom_operators``.
    ``fit_batch`` / ``fit_minibatches`` (and ``fit_stream`` for each of its subsample fits) take ``objective_every=k``: record
    the objective every k iterations (epochs), i = 0, k, 2k, ...; and ``tol``: stop on its relative decrease (``tol`` alone
    means ``objective_every=10``).  The value recorded at iteration i is the objective of the (W, H) that ENTERS iteration i
    -- what ``objective()`` would return at that moment, so the first one is the objective of the initialisation.  It is the
    data term only (1/2 ||V - R||^2, sum D_beta(V | R + eps), or their weighted sums; with transforms of the effective
    problem): the sparsity and inhibition penalties are not part of it.  After the j-th record (j >= 1) the fit has
    converged if ``E[j-1] - E[j] <= tol * E[0]`` (scikit-learn's criterion); that iteration is completed and the fit ends
    with ``converged_ = True``.  A non-finite value ends the fit after its iteration with a RuntimeWarning.  Read-outs after
    every fit: ``objective_history_`` ([n_records, 2]: iteration, value), ``n_iter_``, ``converged_``.  On a backend with
    the objective tap a full-batch record costs one pass over (V, R) inside the H half step, not a reconstruction.
    **kwargs : forwarded to the backend constructor (``reconstruction_mode``, ``device``, ``path``, ``init``,
               ``process_group``)
    """

    def __init__(self, n_atoms: int, atom_shape: Tuple[int, ...], inhibition_range: Union[int, Tuple[int, ...]] = None,
                 backend: Union[str, Backend] = 'hip', logger: logging.Logger = None, verbose: int = 0,
                 use_fused_updates: bool = True, beta_loss: Union[str, float] = 2.,
                 transforms: Union[None, str, _transforms.AtomOperators] = None, **kwargs):
        self._beta = beta_loss_value(beta_loss)
        self.atom_shape = tuple(atom_shape)
        self.n_atoms = n_atoms
        self._transforms = _transforms.check(transforms, self.atom_shape)   # (before anything is built)
        self.n_transforms = 1 if self._transforms is None else _transforms.size(self._transforms)
        k = len(self.atom_shape)
        if inhibition_range is None:
            self._inhibition_range = tuple(a - 1 for a in self.atom_shape)
        elif isinstance(inhibition_range, int):
            self._inhibition_range = (inhibition_range,) * k
        else:
            self._inhibition_range = tuple(inhibition_range)
        assert len(self._inhibition_range) == k
        # parabolic 1-D kernels 1 - (x / (i + 1))^2, x = -i..i  (reference :163)
        self._inhibition_kernels_1D = tuple(1 - (np.arange(-i, i + 1) / (i + 1)) ** 2 for i in self._inhibition_range)
        self._axes_W_normalization = tuple(range(-k, 0))
        self.eps = 1.e-9

        if isinstance(backend, str):
            registry = _backend_registry()
            if backend.lower() not in registry:
                raise KeyError(f'unknown backend {backend!r}; this package provides {sorted(registry)}')
            self._backend = registry[backend.lower()](**kwargs)
        else:
            self._backend = backend

        if self._beta != 2. and not getattr(self._backend, 'supports_beta_loss', False):
            raise NotImplementedError(f'beta_loss={beta_loss!r}: the backend {type(self._backend).__name__} does not '
                                      f'support beta-divergence objectives')
        if self._transforms is not None and not getattr(self._backend, 'supports_transforms', False):
            raise NotImplementedError(f'transforms={transforms!r}: the backend {type(self._backend).__name__} does not '
                                      f'support transform groups')
        if (isinstance(self._transforms, _transforms.AtomOperators)
                and not getattr(self._backend, 'supports_atom_operators', False)):
            raise NotImplementedError(f'transforms={transforms!r}: the backend {type(self._backend).__name__} does not '
                                      f'support atom operators')

        self._logger = logger if logger is not None else logging.getLogger(self.__class__.__name__)
        self._logger.setLevel([logging.ERROR, logging.WARNING, logging.INFO, logging.DEBUG][verbose])
        self._use_fused = bool(use_fused_updates)
        self._use_schedules = bool(use_fused_updates)   # mini-batch epochs as one backend call where the backend can
        self._iteration_acc = None
        self._weighted = False   # the current fit has weights (set by every fit)
        self._weights = None

        self._W = None
        self._W_eff = None   # with transforms: the M * T effective atoms, expanded from W after every change of W
        self._H = None
        self._V = None
        self._shuffle_idx = None
        self.objective_history_ = np.empty((0, 2))
        self.n_iter_ = 0
        self.converged_ = False
        self._objective_buf = None   # the tap's per-sample buffer of the current fit
        self.pursuit_history_ = np.empty((0, 3))   # of the last pursue_detections
        self.relocation_history_ = np.empty((0, 3))   # of the last relocate_detections
        self.solve_history_ = np.empty((0, 2))   # of the last solve_detections: (iteration, kkt) of its checks
        self.solve_n_iter_ = 0
        self.solve_converged_ = False

    # -- read-outs (reference :188-215) ---------------------------------------------------------------------
    @property
    def W(self) -> np.ndarray:
        return self._backend.to_ndarray(self._W)

    @property
    def H(self) -> np.ndarray:
        H = self._backend.to_ndarray(self._H)
        H = H if self._shuffle_idx is None else H[np.argsort(self._shuffle_idx)]
        if self._transforms is not None:
            H = H.reshape((H.shape[0], self.n_atoms, self.n_transforms) + H.shape[2:])
        return H

    @property
    def transforms(self) -> Union[None, str, _transforms.AtomOperators]:
        """The transform group or the atom operators (None: shifts only)."""
        return self._transforms

    @property
    def transformed_atoms(self) -> np.ndarray:
        """[M, T, C, *A]: atom m in orientation t, ``T_t(W[m])`` (T = 1 without transforms)."""
        W = self._backend.to_ndarray(self._W_dict)
        return W.reshape((self.n_atoms, self.n_transforms) + W.shape[1:])

    @property
    def V(self) -> np.ndarray:
        return self._V if self._shuffle_idx is None else self._V[np.argsort(self._shuffle_idx)]

    @property
    def R(self) -> np.ndarray:
        return self._backend.to_ndarray(self._backend.reconstruct(self._W_dict, self._H))

    def R_partial(self, i_atom: int) -> np.ndarray:
        """Atom ``i_atom``'s contribution to R (with transforms: in all its orientations)."""
        if self._transforms is None:
            return self._backend.to_ndarray(self._backend.partial_reconstruct(self._W, self._H, i_atom))
        eff = slice(i_atom * self.n_transforms, (i_atom + 1) * self.n_transforms)
        return self._backend.to_ndarray(self._backend.reconstruct(self._W_eff[eff], self._H[:, eff]))

    @property
    def _W_dict(self):
        """The dictionary the H side works with: W, or with transforms the M * T effective atoms."""
        return self._W if self._transforms is None else self._W_eff

    def _expand_W(self) -> None:
        """W has changed: expand it into the effective atoms again (no-op without transforms)."""
        if self._transforms is not None:
            self._backend.expand_W(self._W, self._transforms, self._W_eff)

    @property
    def beta_loss(self) -> float:
        """beta of the objective D_beta (2: Frobenius)."""
        return self._beta

    @property
    def _plain_frobenius(self) -> bool:
        """The objective is the plain Frobenius one (beta == 2, no weights) of a model without transforms: the only one the
        reference's own lines, the backend's Frobenius-only primitives and the one-call schedules compute."""
        return self._beta == 2. and not self._weighted and self._transforms is None

    def _objective(self, **kwargs) -> dict:
        """Keyword arguments of a backend hook, plus ``beta`` and ``eps`` for any objective but the plain Frobenius one
        (for that one the hooks are called exactly as on a Frobenius-only backend)."""
        if not self._plain_frobenius:
            kwargs.update(beta=self._beta, eps=self.eps)
        return kwargs

    def _energy_function(self) -> float:
        return self._backend.reconstruction_energy(self._V, self._W_dict, self._H, **self._objective())

    def objective(self) -> float:
        """The objective of the current (W, H): 1/2 ||V - R||^2, sum D_beta(V | R + eps), or the weighted sum of either --
        the data term only, without the sparsity and inhibition penalties."""
        return self._energy_function()

    # -- detections -----------------------------------------------------------------------------------------------------
    _SUPPRESS = ('atom', 'transforms', 'all')

    def detections(self, threshold: float = 0., min_distance: Union[None, int, Tuple[int, ...]] = None,
                   suppress: str = 'atom', max_per_sample: Optional[int] = None) -> Detections:
        """Where each atom occurs: the entries of ``H`` above ``threshold`` (strictly) that no entry within
        ``min_distance`` on every shift axis suppresses -- a larger one, or an equal one with the lower C-order index, so a
        plateau has one winner per neighbourhood.  Neighbourhoods end at the border of the plane in every reconstruction
        mode.  NaN is never a detection.

        min_distance : ``None`` (the model's ``inhibition_range``: the neighbourhood lateral inhibition acts on), an int or
                       one int per shift axis, >= 0
        suppress : what competes for a location -- ``'atom'`` each effective atom with itself only, ``'transforms'`` the T
                   orientations of one atom, ``'all'`` every atom and orientation
        max_per_sample : keep only each sample's strongest k (ties: the lower C-order index first)

        On a backend with ``find_peaks`` the search runs on the device and only the list of detections is copied; any
        other backend's ``H`` is searched on the host."""
        if self._H is None:
            raise RuntimeError('detections() needs a fitted model: call fit first')
        _args.finite_number('threshold', threshold, '>= 0')
        k = len(self.atom_shape)
        if min_distance is None:
            radius = self._inhibition_range
        elif _args.is_int(min_distance):
            radius = (min_distance,) * k
        elif isinstance(min_distance, (tuple, list)) and len(min_distance) == k:
            radius = tuple(min_distance)
        else:
            raise ValueError(f'min_distance must be None, an int or {k} ints, not {min_distance!r}')
        if any(not _args.is_int(r) or r < 0 for r in radius):
            raise ValueError(f'min_distance must be >= 0 on every axis, not {min_distance!r}')
        radius = tuple(int(r) for r in radius)
        if not isinstance(suppress, str) or suppress not in self._SUPPRESS:
            raise ValueError(f'suppress must be one of {self._SUPPRESS}, not {suppress!r}')
        if suppress == 'transforms' and self._transforms is None:
            raise ValueError("suppress='transforms' needs a model with transforms")
        _args.int_at_least('max_per_sample', max_per_sample, 0, none_ok=True)
        shape = tuple(int(x) for x in self._H.shape)   # [local samples, M * T, *shift]
        T = self.n_transforms
        group = {'atom': 1, 'transforms': T, 'all': shape[1]}[suppress]
        hook = getattr(self._backend, 'find_peaks', None)
        if hook is not None:
            idx, val = hook(self._H, float(threshold), radius, group)
        else:
            idx, val = find_peaks_numpy(self._backend.to_ndarray(self._H), float(threshold), radius, group)
        at = np.unravel_index(np.asarray(idx, dtype=np.int64), shape)
        sample = at[0].astype(np.int64)
        if self._shuffle_idx is not None:
            # (the H property shows internal sample a[i] at place i, a = argsort(shuffle): undo it, keep the C order)
            place = np.empty(shape[0], dtype=np.int64)
            place[np.argsort(self._shuffle_idx)] = np.arange(shape[0])
            sample = place[sample]
            order = np.argsort(sample, kind='stable')
            sample, val, at = sample[order], val[order], tuple(a[order] for a in at)
        if max_per_sample is not None:
            # each sample's strongest first, ties in C order; the survivors stay in C order
            by_strength = np.lexsort((np.arange(len(val)), -val.astype(np.float64), sample))
            first = np.searchsorted(sample, sample[by_strength], side='left')   # (sample is ascending)
            keep = np.sort(by_strength[np.arange(len(val)) - first < max_per_sample])
            sample, val, at = sample[keep], val[keep], tuple(a[keep] for a in at)
        sample = sample + int(getattr(self._backend, 'shard', (0, 0))[0])
        shift = np.stack([a.astype(np.int64) for a in at[2:]], axis=1).reshape(len(val), k)
        return Detections(sample=sample, atom=(at[1] // T).astype(np.int64), transform=(at[1] % T).astype(np.int64),
                          shift=shift, origin=shift - self._origin_offset(), strength=val)

    # -- detections rendered and refitted -------------------------------------------------------------------------------
    @property
    def _mode(self) -> str:
        """The backend's reconstruction mode ('valid' for a backend that does not say)."""
        return getattr(self._backend, '_reconstruction_mode', 'valid')

    def _origin_offset(self) -> np.ndarray:
        """[k]: ``shift - origin`` of a detection, ``atom_shape - 1`` in 'valid' mode and 0 in the others."""
        return np.array([a - 1 if self._mode == 'valid' else 0 for a in self.atom_shape], dtype=np.int64)

    def _plain_frobenius_only(self, who: str) -> bool:
        """The refusal the list operations share: ``who`` works on the plain Frobenius objective.  Returns whether the
        model is fitted and not a volume -- the two ``_events_of`` refuses next, with messages of its own."""
        served = self._H is not None and len(self.atom_shape) != 3
        if served and (self._beta != 2. or self._weighted):
            raise NotImplementedError(f'{who} covers the plain Frobenius objective (beta_loss 2, no weights)')
        return served

    def _events_of(self, det, distinct: bool):
        """The events of ``det`` in the backend's terms -- (internal local sample, plane of the effective dictionary, shift,
        strength in the model's element type) -- after the checks: the inverse of what ``detections()`` applies to the
        sample (shard offset, shuffle) and to the plane (atom * T + transform)."""
        if self._H is None:
            raise RuntimeError('the detections of a model need a fitted model: call fit first')
        k = len(self.atom_shape)
        if k == 3:
            raise NotImplementedError('detections are rendered and refitted on 1 or 2 shift axes, not volumes')
        shape = tuple(int(x) for x in self._H.shape)   # [local samples, M * T, *shift]
        T = self.n_transforms
        cols = [np.asarray(getattr(det, name)) for name in ('sample', 'atom', 'transform', 'shift', 'strength')]
        K = len(cols[0])
        for name, c in zip(('sample', 'atom', 'transform', 'shift'), cols):
            if c.dtype.kind not in 'iu':
                raise ValueError(f'detections: {name} must hold integers, not {c.dtype}')
        sample, atom, transform = (c.astype(np.int64).reshape(-1) for c in cols[:3])
        if cols[3].size != K * k or len(atom) != K or len(transform) != K or cols[4].size != K:
            raise ValueError('detections: one row per detection in sample, atom, transform, shift and strength')
        shift = cols[3].astype(np.int64).reshape(K, k)
        if cols[4].dtype.kind not in 'iuf':
            raise ValueError(f'detections: strength must hold real numbers, not {cols[4].dtype}')
        with np.errstate(over='ignore'):
            strength = cols[4].reshape(-1).astype(self._V.dtype)
        n0 = int(getattr(self._backend, 'shard', (0, 0))[0])
        local = sample - n0
        if np.any((local < 0) | (local >= shape[0])):
            raise ValueError(f'detections: samples outside the samples [{n0}, {n0 + shape[0]}) of this model (rank)')
        if np.any((atom < 0) | (atom >= self.n_atoms)) or np.any((transform < 0) | (transform >= T)):
            raise ValueError(f'detections: atoms outside [0, {self.n_atoms}) or transforms outside [0, {T})')
        if np.any((shift < 0) | (shift >= np.asarray(shape[2:], dtype=np.int64))):
            raise ValueError(f'detections: shifts outside the shift shape {shape[2:]}')
        if not np.all(np.isfinite(strength)) or np.any(strength < 0):
            raise ValueError('detections: strengths must be finite and >= 0')
        if distinct and K and len(np.unique(np.column_stack([sample, atom, transform, shift]), axis=0)) != K:
            raise ValueError('detections: a refit needs distinct (sample, atom, transform, shift)')
        if self._shuffle_idx is not None:
            local = np.argsort(self._shuffle_idx)[local]   # (the H property shows internal sample a[i] at place i)
        return local, atom * T + transform, shift, strength

    def _local_V(self) -> np.ndarray:
        """This rank's samples on the host, in the backend's order."""
        n0, n = int(getattr(self._backend, 'shard', (0, 0))[0]), int(self._H.shape[0])
        return self._V if len(self._V) == n else self._V[n0:n0 + n]

    def _rows_to_detections(self, sample, plane, shift, strength) -> Detections:
        """The inverse of ``_events_of``: rows in the backend's terms as the ``Detections`` the caller sees."""
        sample = np.asarray(sample, dtype=np.int64)
        if self._shuffle_idx is not None:   # (internal sample a[i] is shown at place i)
            place = np.empty(int(self._H.shape[0]), dtype=np.int64)
            place[np.argsort(self._shuffle_idx)] = np.arange(int(self._H.shape[0]))
            sample = place[sample]
        sample = sample + int(getattr(self._backend, 'shard', (0, 0))[0])
        plane = np.asarray(plane, dtype=np.int64)
        shift = np.asarray(shift, dtype=np.int64).reshape(len(sample), len(self.atom_shape))
        T = self.n_transforms
        return Detections(sample=sample, atom=plane // T, transform=plane % T, shift=shift,
                          origin=shift - self._origin_offset(), strength=np.asarray(strength))

    def _with_strengths(self, det, shift, strength) -> Detections:
        """The rows of ``det`` (any object with its columns; ``shift`` is theirs, checked) with new strengths."""
        as_rows = lambda x: np.asarray(x).astype(np.int64).reshape(len(strength))   # noqa: E731
        return Detections(sample=as_rows(det.sample), atom=as_rows(det.atom), transform=as_rows(det.transform),
                          shift=shift, origin=shift - self._origin_offset(), strength=strength)

    def _host_problem(self, W=None):
        """(dictionary on the host, sample shape, local samples, mode): what every function of events_host.py takes first.
        ``W``: the effective dictionary unless given."""
        return (self._backend.to_ndarray(self._W_dict if W is None else W), self._V.shape[2:], int(self._H.shape[0]),
                self._mode)

    def _on_events(self, hook_name: str, fallback: Callable, rows, *more, **kw):
        """The backend's hook ``hook_name`` on the rows of ``_events_of``, or on a backend without it the function
        ``fallback`` of events_host.py, which takes the host problem, the rows, this rank's samples and the same rest."""
        hook = getattr(self._backend, hook_name, None)
        if hook is not None:
            return hook(self._V, self._W_dict, *rows, *more, **kw)
        return fallback(*self._host_problem(), *rows, self._local_V(), *more, **kw)

    def reconstruct_detections(self, det) -> np.ndarray:
        """What the detections ``det`` (a ``Detections``, or any object with its sample, atom, transform, shift and
        strength) explain: the reconstruction of the activations that hold the strengths at the detections and zero
        elsewhere, in the order and shape of ``R``.  Duplicate rows add up.  On a backend with ``render_events`` the list is
        rendered on the device, without a dense H; any other backend's is rendered on the host."""
        sample, plane, shift, strength = self._events_of(det, distinct=False)
        hook = getattr(self._backend, 'render_events', None)
        if hook is not None:
            return self._backend.to_ndarray(hook(self._W_dict, sample, plane, shift, strength))
        return events_numpy(*self._host_problem(), sample, plane, shift, strength)

    def refit_detections(self, det, n_iterations: int = 50, sparsity_H: float = 0.) -> Detections:
        """The detections with their strengths refitted: ``n_iterations`` multiplicative updates of the strengths alone, on
        the fixed support ``det`` and the fixed dictionary, against the model's own V -- the H half step without
        inhibition on activations that are zero off the support.  It removes the shrinkage the strengths carry from a fit
        under ``sparsity_H`` or inhibition (and from the sub-threshold activations ``detections()`` dropped).  The rows must
        be distinct; a strength of 0 stays 0.  The plain Frobenius objective only."""
        self._plain_frobenius_only('refit_detections')
        _args.int_at_least('n_iterations', n_iterations, 0)
        _args.finite_number('sparsity_H', sparsity_H, '>= 0')
        sample, plane, shift, strength = self._events_of(det, distinct=True)
        hook = getattr(self._backend, 'refit_events', None)
        if hook is not None:
            new = self._backend.to_ndarray(hook(self._V, self._W_dict, sample, plane, shift, strength, int(n_iterations),
                                                sparsity=float(sparsity_H), eps=self.eps))
        else:
            new = events_numpy(*self._host_problem(), sample, plane, shift, strength, V=self._local_V(),
                               n_iterations=int(n_iterations), sparsity=float(sparsity_H), eps=self.eps)
        return self._with_strengths(det, shift, new)

    def solve_detections(self, det, tol: float = 1e-8, max_iterations: int = 10000) -> Detections:
        """The detections with the strengths that MINIMISE the objective on the fixed support ``det`` and the fixed
        dictionary, against the model's own V: the non-negative least-squares strengths of the list, the orthogonal step of
        orthogonal matching pursuit.  With phi_i the occurrence of row i the objective is the quadratic
        ``1/2 ||V||^2 - c'h + 1/2 h'Gh``, ``c_i = <phi_i, V>`` and ``G_ij = <phi_i, phi_j>`` (sparse: rows couple only where
        their footprints meet); it is minimised over ``h >= 0`` in float64 by an accelerated projected gradient method on
        the list alone, from the strengths of ``det``.  Unlike ``refit_detections`` a strength of 0 may grow, and there is a
        stopping rule: with ``g = Gh - c``, ``pg_i = g_i`` where ``h_i > 0`` and ``min(g_i, 0)`` where ``h_i = 0``, it stops at
        ``kkt = max |pg| / max |c| <= tol`` or after ``max_iterations`` steps (0: the start, projected, with its kkt).  A
        row without a pixel inside the sample gets 0.  The returned strengths are the solution rounded once to the
        model's element type.  Read-outs: ``solve_history_`` ([checks, 2]: iteration, kkt), ``solve_n_iter_``,
        ``solve_converged_`` -- a run that ends unconverged returns its last iterate and says so there.  The rows must be
        distinct; the plain Frobenius objective only.  On a backend with ``solve_events`` everything runs on the device.
        With a process group every rank solves its own samples: the call is not collective."""
        self._plain_frobenius_only('solve_detections')
        self._check_solve_args(tol, max_iterations)
        sample, plane, shift, strength = self._events_of(det, distinct=True)
        hook = getattr(self._backend, 'solve_events', None)
        if hook is not None:
            new, info = hook(self._V, self._W_dict, sample, plane, shift, strength, float(tol), int(max_iterations))
            new = np.asarray(self._backend.to_ndarray(new), dtype=np.float64)
        else:
            G, c = events_gram_numpy(*self._host_problem(), sample, plane, shift, V=self._local_V(), sparse=True)
            new, info = events_solve_numpy(G, c, strength, float(tol), int(max_iterations))
        self.solve_history_ = np.asarray(info['history'], dtype=np.float64).reshape(-1, 2)
        self.solve_n_iter_ = int(info['iterations'])
        self.solve_converged_ = bool(info['converged'])
        return self._with_strengths(det, shift, new.astype(self._V.dtype))

    def detection_errors(self, det, noise: Optional[float] = None, max_component: int = 2048) -> Tuple[np.ndarray, np.ndarray]:
        """(stderr [K], vif [K]) in float64: how well the strengths of ``det`` are determined.  Meant for the output of
        ``solve_detections``: at that solution the strengths of the active rows ``A = {i : strength_i > 0}`` are the
        least-squares estimate on their support, so ``Cov(h_A) = sigma^2 (G_AA)^-1`` with ``G_ij = <phi_i, phi_j>`` the Gram
        matrix of the occurrences.  ``stderr_i = sigma sqrt(((G_AA)^-1)_ii)`` is the standard error of a strength --
        ``z = det.strength / stderr`` is a threshold without units -- and ``vif_i = G_ii ((G_AA)^-1)_ii >= 1`` the variance
        inflation: how much the neighbours of a row blur it, exactly 1 for a row that touches no other active row.  G is
        sparse and ``G_AA`` block diagonal over the connected components of its coupling graph, so the diagonal of the inverse
        is exact: one small dense factorisation per component.  A row of strength 0 gets NaN in both; the rows of a component
        that is numerically singular (two orientations of a symmetric atom at one place are collinear) get +inf.

        noise : the standard deviation sigma of the data, finite and > 0.  ``None`` estimates it from the residual of the
                list, ``sigma^2 = ||V - R(det)||^2 / (n_obs - K_A)`` with ``n_obs`` the entries of this model's (rank's)
                samples and ``K_A`` the active rows; ValueError when ``n_obs <= K_A``.
        max_component : the largest component that is inverted (int >= 1); a larger one raises ValueError.

        Read-out: ``errors_info_``, a dict with noise, dof, residual_energy, n_active, n_components, largest_component,
        n_singular and rounds (of the component search).  The rows must be distinct; the plain Frobenius objective only.
        ``H``, ``W`` and ``det`` are not touched.  On a backend with ``event_errors`` everything runs on the device.  With a
        process group every rank uses its own samples and the call is not collective: a sigma shared by the ranks is the
        caller's to pass in as ``noise``."""
        self._plain_frobenius_only('detection_errors')
        _args.finite_number('noise', noise, '> 0', none_ok=True)
        _args.int_at_least('max_component', max_component, 1)
        sample, plane, shift, strength = self._events_of(det, distinct=True)
        hook = getattr(self._backend, 'event_errors', None)
        if hook is not None:
            d, b, energy, info = hook(self._V, self._W_dict, sample, plane, shift, strength, int(max_component))
            d, b = (np.asarray(self._backend.to_ndarray(x), dtype=np.float64) for x in (d, b))
            row_size = np.asarray(self._backend.to_ndarray(info['row_size']))
        else:
            V = np.asarray(self._local_V(), dtype=np.float64)
            G, c = events_gram_numpy(*self._host_problem(), sample, plane, shift, V=V, sparse=True)
            h = strength.astype(np.float64)
            d, info = events_inverse_diag_numpy(G, h > 0, int(max_component))
            row_of = np.repeat(np.arange(len(h)), np.diff(G[0]))
            b = np.zeros(len(h))
            b[row_of[row_of == G[1]]] = G[2][row_of == G[1]]
            energy = max(float(np.sum(V * V) - 2. * (c @ h) + np.sum(G[2] * h[row_of] * h[G[1]])), 0.)
            row_size = info['row_size']
        n_obs = int(self._H.shape[0]) * int(np.prod(self._V.shape[1:]))
        dof = n_obs - int(info['n_active'])
        if noise is None:
            if dof <= 0:
                raise ValueError(f'detection_errors: {n_obs} observations do not determine the noise of '
                                 f'{info["n_active"]} active rows: pass noise=')
            sigma = math.sqrt(energy / dof)
        else:
            sigma = float(noise)
        with np.errstate(invalid='ignore'):
            stderr = sigma * np.sqrt(d)
            vif = np.where(row_size == 1, 1., b * d)
        self.errors_info_ = dict(noise=sigma, dof=dof, residual_energy=float(energy), n_active=int(info['n_active']),
                                 n_components=int(info['n_components']), largest_component=int(info['largest_component']),
                                 n_singular=int(info['n_singular']), rounds=int(info['rounds']))
        return stderr, vif

    @staticmethod
    def _check_solve_args(tol, max_iterations) -> None:
        _args.finite_number('tol', tol, '> 0')
        _args.int_at_least('max_iterations', max_iterations, 0)

    def _list_strengths(self, who: str, strengths, n_iterations, sparsity_H, tol, max_iterations):
        """det -> det with the strengths of a round of ``who``: ``refit_detections`` ('mu') or ``solve_detections``
        ('solve'), after the checks of the keyword."""
        if strengths == 'mu':
            return lambda det: self.refit_detections(det, n_iterations, sparsity_H)
        if strengths != 'solve':
            raise ValueError(f"strengths must be 'mu' or 'solve', not {strengths!r}")
        _args.finite_number('sparsity_H', sparsity_H, '>= 0')
        if sparsity_H != 0:
            raise ValueError(f"{who}: strengths='solve' minimises the objective without a sparsity term: sparsity_H must "
                             f'be 0, not {sparsity_H!r}')
        self._check_solve_args(tol, max_iterations)
        return lambda det: self.solve_detections(det, tol, max_iterations)

    def detection_gains(self, det) -> np.ndarray:
        """[K] float64: what each detection of ``det`` explains -- the objective 1/2 ||V - R||^2 of the list without the row
        minus that of the list, R being ``reconstruct_detections(det)``: ``h a + h^2 b / 2`` with phi the row's occurrence
        (all its images, clipped to the sample), ``a = <phi, V - R>`` and ``b = ||phi||^2``.  Positive where the row lowers
        the objective; after a refit to convergence ``a = 0`` and the gain is ``h^2 b / 2``.  Unlike the strength it is in
        the units of the objective for every atom.  Duplicate rows are scored each against the whole list.  On a backend
        with ``event_gains`` the list is rendered and scored on the device and only the K gains are copied.  The plain
        Frobenius objective only."""
        self._plain_frobenius_only('detection_gains')
        rows = self._events_of(det, distinct=False)
        return np.asarray(self._on_events('event_gains', events_gain_numpy, rows), dtype=np.float64)

    def prune_detections(self, det, min_gain: float, n_iterations: int = 50, sparsity_H: float = 0.,
                         max_rounds: int = 100, strengths: str = 'mu', tol: float = 1e-8,
                         max_iterations: int = 10000) -> Tuple[Detections, np.ndarray]:
        """Backward elimination: the rows of ``det`` the data needs, refitted, and their gains.  Each round refits the
        strengths (``refit_detections`` with ``n_iterations`` and ``sparsity_H``), scores the rows (``detection_gains``) and
        takes those with a gain below ``min_gain`` as candidates.  Per sample the candidates are walked in ascending gain
        (ties in row order) and dropped unless the bounding box of their occurrence in the sample meets that of a candidate
        already dropped in this round: rows with disjoint footprints have independent gains, so dropping them together is
        exact, and overlapping ones are scored again in the next round, after a refit without their neighbour.  It stops
        when a round finds no candidate or after ``max_rounds`` rounds of dropping; ``max_rounds=0`` is a refit with its
        gains.  The rows are chosen on the host -- the list is small; refit, render and gains run where the backend runs
        them.  The rows must be distinct; the plain Frobenius objective only.  With ``strengths='solve'`` the strengths of
        every round are ``solve_detections(tol=, max_iterations=)``' -- the gains are then those of the true minimiser;
        ``n_iterations`` is unused and ``sparsity_H`` must be 0."""
        self._plain_frobenius_only('prune_detections')
        _args.finite_number('min_gain', min_gain)
        _args.int_at_least('max_rounds', max_rounds, 0)
        fitted = self._list_strengths('prune_detections', strengths, n_iterations, sparsity_H, tol, max_iterations)
        rounds = 0
        while True:
            det = fitted(det)
            gains = self.detection_gains(det)
            if rounds >= max_rounds:
                break
            lo, hi = event_boxes(det.shift, self.atom_shape, self._V.shape[2:], tuple(int(x) for x in self._H.shape[2:]),
                                 self._mode)
            keep = np.ones(len(det), dtype=bool)
            candidates = np.flatnonzero(gains < min_gain)
            dropped = {}   # per sample: the boxes dropped in this round
            for e in candidates[np.argsort(gains[candidates], kind='stable')]:
                boxes = dropped.setdefault(int(det.sample[e]), [])
                if any(np.all(np.maximum(lo[e], a) < np.minimum(hi[e], b)) for a, b in boxes):
                    continue
                boxes.append((lo[e], hi[e]))
                keep[e] = False
            if keep.all():
                break
            det = Detections(**{f.name: getattr(det, f.name)[keep] for f in dataclasses.fields(Detections)})
            rounds += 1
        return det, gains

    def pursue_detections(self, min_gain: float, max_events: Optional[int] = None, max_rounds: int = 100,
                          refit_iterations: int = 10, n_iterations: int = 50, sparsity_H: float = 0.,
                          start=None, strengths: str = 'mu', tol: float = 1e-8,
                          max_iterations: int = 10000) -> Tuple[Detections, np.ndarray]:
        """Forward selection: the detections the data asks for, found without a dense fit of H -- convolutional matching
        pursuit in its batched, locally greedy form -- and their gains, the pair ``prune_detections`` returns.  It works on
        the model's own V and its current dictionary; to detect in new data with a learnt dictionary call
        ``fit_batch(V_new, n_iterations=0, keep_W=True)`` first.  The list starts as ``start`` (a ``Detections`` with
        distinct rows) or empty.  Each round takes the residual ``V - R`` of the list, R being its render, and scores
        every possible row: with phi, ``a = <phi, V - R>`` and ``b = ||phi||^2`` as in ``detection_gains``, adding the row at
        its best strength ``a / b`` lowers the objective by ``a^2 / (2 b)`` (0 where ``a <= 0``, and for the rows already in
        the list).  The candidates are the entries of that gain map above ``min_gain`` that are the largest within
        ``atom_shape - 1`` on every shift axis over all atoms and orientations; per sample they are walked in descending gain
        (ties in index order) and kept unless the bounding box of their occurrence in the sample meets that of a candidate
        already kept in this round -- which the spacing alone does not rule out for wrapped and mirrored occurrences.  Rows
        with disjoint footprints do not interact, so adding them together is exact: the objective falls by the sum of
        their gains.  The map only ranks; the strength and the gain of a kept row are computed again in double, and a row
        whose exact gain is not above ``min_gain`` is dropped.  The list is then refitted for ``refit_iterations`` steps (the
        step of ``refit_detections``; 0: not at all) and the next round begins.  It stops when a round keeps nothing, after
        ``max_rounds`` rounds or with ``max_events`` rows (the last round then keeps its highest gains).  At the end the
        list is refitted once more (``refit_detections`` with ``n_iterations`` and ``sparsity_H``) and scored
        (``detection_gains``).  ``min_gain`` is in the units of the objective, the same for every atom.  Read-out:
        ``pursuit_history_`` ([rounds, 3]: candidates found, rows added, the sum of their exact gains).  On a backend with
        ``pursue_events`` the map, its peaks and the scores are computed on the device; only the candidates (index, gain)
        and the kept rows are copied.
        The model's dense ``H`` is left as it is.  The plain Frobenius objective only.  With a process group every rank
        pursues its own samples: the call is not collective.
        With ``strengths='solve'`` the list's strengths after every round, and at the end, are
        ``solve_detections(tol=, max_iterations=)``' -- orthogonal matching pursuit; ``refit_iterations`` and
        ``n_iterations`` are unused and ``sparsity_H`` must be 0."""
        self._plain_frobenius_only('pursue_detections')
        _args.finite_number('min_gain', min_gain, '> 0')
        _args.int_at_least('max_rounds', max_rounds, 0)
        _args.int_at_least('refit_iterations', refit_iterations, 0)
        _args.int_at_least('n_iterations', n_iterations, 0)
        if max_events is not None:   # (None is no limit; the message does not offer it)
            _args.int_at_least('max_events', max_events, 0)
        _args.finite_number('sparsity_H', sparsity_H, '>= 0')
        fitted = self._list_strengths('pursue_detections', strengths, n_iterations, sparsity_H, tol, max_iterations)
        solve = (float(tol), int(max_iterations)) if strengths == 'solve' else None
        k = len(self.atom_shape)
        if start is None:
            start = Detections(sample=np.zeros(0, dtype=np.int64), atom=np.zeros(0, dtype=np.int64),
                               transform=np.zeros(0, dtype=np.int64), shift=np.zeros((0, k), dtype=np.int64),
                               origin=np.zeros((0, k), dtype=np.int64), strength=np.zeros(0))
        rows = self._events_of(start, distinct=True)
        max_events = None if max_events is None else int(max_events)
        more = {} if solve is None else {'solve': solve}   # (a hook without the keyword keeps serving strengths='mu')
        *rows, self.pursuit_history_ = self._on_events(
            'pursue_events', pursuit_numpy, rows, float(min_gain), max_events=max_events, max_rounds=int(max_rounds),
            refit_iterations=int(refit_iterations), eps=self.eps, **more)
        det = fitted(self._rows_to_detections(*rows))
        return det, self.detection_gains(det)

    # -- detections moved: the landscape of the neighbouring shifts ----------------------------------------------------
    def _landscape(self, det, distinct: bool, who: str):
        """(a, b) ``[K, 3^k]`` float64 of the rows of ``det``, after the refusals and checks ``who`` shares with
        ``detection_gains``, and the rows in the backend's terms."""
        self._plain_frobenius_only(who)
        rows = self._events_of(det, distinct=distinct)
        a, b = self._on_events('event_landscape', events_landscape_numpy, rows)
        return np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rows

    def detection_landscape(self, det) -> Tuple[np.ndarray, np.ndarray]:
        """(a, b), each ``[K] + (3,) * k`` float64: every row of ``det`` scored at its neighbouring shifts ``shift + delta``,
        delta in {-1, 0, 1} per shift axis (index ``delta + 1``), with everything else in the list held fixed.  With R =
        ``reconstruct_detections(det)`` and ``d = V - R + h phi`` the residual of the list without the row, ``a = <phi', d>``
        and ``b = ||phi'||^2`` for the row's atom at the neighbouring shift (phi': all its images, clipped to the sample).  A
        row there at its best strength ``a / b`` would take ``a^2 / (2 b)`` off the objective of the list without the row
        (for ``a > 0``).  Zeros for a neighbour outside the shift shape: nothing wraps from one end of the shift range to the
        other.  At the centre ``h (a - h b) + h^2 b / 2`` is the row's ``detection_gains``.  Duplicate rows put back only
        themselves.  On a backend with ``event_landscape`` the list is rendered and scored on the device and only the
        ``2 K 3^k`` numbers are copied.  The plain Frobenius objective only."""
        a, b, _ = self._landscape(det, False, 'detection_landscape')
        shape = (len(a),) + (3,) * len(self.atom_shape)
        return a.reshape(shape), b.reshape(shape)

    def refine_detections(self, det) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(offset ``[K, k]`` float64, gain ``[K]`` float64, is_peak ``[K]`` bool): sub-pixel positions from
        ``detection_landscape``.  With ``g = a^2 / (2 b)`` (0 where ``a <= 0`` or ``b <= 0``), ``gain`` is g at the row's own
        shift.  Per shift axis i a parabola goes through g at delta = -1, 0, +1 along that axis: with ``c = g- - 2 g0 + g+``,
        where ``g0 >= max(g-, g+)`` and ``c < 0`` its vertex ``offset_i = (g- - g+) / (2 c)``, clipped to [-1/2, 1/2];
        elsewhere -- the row is not a maximum along the axis, or sits where the axis ends -- ``offset_i = 0`` and ``is_peak``
        is False for the row.  ``det.origin + offset`` is the sub-pixel origin of the atom.  The rows need not be distinct.
        The plain Frobenius objective only."""
        a, b, _ = self._landscape(det, False, 'refine_detections')
        k = len(self.atom_shape)
        g = landscape_gains(a, b).reshape((len(a),) + (3,) * k)
        centre = (slice(None),) + (1,) * k
        g0 = g[centre]
        offset, is_peak = np.zeros((len(a), k)), np.ones(len(a), dtype=bool)
        for i in range(k):
            lo, hi = (g[centre[:1 + i] + (j,) + centre[2 + i:]] for j in (0, 2))
            c = lo - 2. * g0 + hi
            ok = (g0 >= np.maximum(lo, hi)) & (c < 0)
            offset[:, i] = np.where(ok, np.clip(0.5 * (lo - hi) / np.where(ok, c, -1.), -0.5, 0.5), 0.) + 0.
            is_peak &= ok
        return offset, g0.copy(), is_peak

    def relocate_detections(self, det, n_iterations: int = 50, sparsity_H: float = 0., max_rounds: int = 100,
                            min_improvement: float = 0., strengths: str = 'mu', tol: float = 1e-8,
                            max_iterations: int = 10000) -> Tuple[Detections, np.ndarray]:
        """Local search over the shifts: the rows of ``det`` moved to where the data explains them better, refitted, and
        their gains -- the third list operation beside ``pursue_detections`` (grow) and ``prune_detections`` (shrink), and
        what it returns is what they return.  Each round refits the strengths (``refit_detections`` with ``n_iterations`` and
        ``sparsity_H``) and takes the landscape (``detection_landscape``).  For a row of strength h, with ``g = a^2 / (2 b)``,
        ``improvement = max over the neighbours of g - (h a_e + h^2 b_0 / 2)``, ``a_e = a_0 - h b_0``: what the objective falls
        by when the row hops to its best neighbour at the strength ``a / b`` there.  The candidates are the rows with
        ``improvement > min_improvement`` whose best neighbour has ``g > 0`` -- a row the data supports nowhere around it
        stays where it is, even with a negative gain of its own: dropping it is ``prune_detections``' part.  Per sample the
        candidates are walked in descending improvement (ties in row order) and hop
        -- to the neighbour of the lowest index among equal ones, ``atom`` and ``transform`` unchanged -- unless the bounding
        box of the old and the new occurrence together meets that of a hop already made in this round (rows with disjoint
        footprints do not interact, so their hops together are exact; the others are scored again next round), or the
        target is already a row of the list (the list stays distinct).  It stops when a round makes no hop or after
        ``max_rounds`` rounds of hopping; ``max_rounds=0`` is a refit with its gains.  Read-out: ``relocation_history_``
        ([rounds, 3]: candidates, hops, the sum of the hops' improvements).  The hops are chosen on the host; refit, render
        and landscape run where the backend runs them.  The rows must be distinct; the plain Frobenius objective only.  With
        a process group every rank moves the rows of its own samples: the call is not collective.  With
        ``strengths='solve'`` the strengths of every round are ``solve_detections(tol=, max_iterations=)``';
        ``n_iterations`` is unused and ``sparsity_H`` must be 0."""
        self._plain_frobenius_only('relocate_detections')
        _args.finite_number('min_improvement', min_improvement, '>= 0')
        _args.int_at_least('max_rounds', max_rounds, 0)
        fitted = self._list_strengths('relocate_detections', strengths, n_iterations, sparsity_H, tol, max_iterations)
        history, rounds = [], 0
        while True:
            det = fitted(det)
            if rounds >= max_rounds:
                break
            a, b, (sample, plane, shift, strength) = self._landscape(det, True, 'relocate_detections')
            hopped, target, h, n_candidates, total = relocation_hops(
                sample, plane, shift, strength, a, b, self.atom_shape, self._V.shape[2:],
                tuple(int(x) for x in self._H.shape[2:]), self._mode, float(min_improvement))
            history.append((n_candidates, len(hopped), total))
            if not len(hopped):
                break
            shift, strength = np.array(det.shift, dtype=np.int64).reshape(len(det), -1), np.array(det.strength)
            shift[hopped], strength[hopped] = target, h.astype(strength.dtype)
            det = dataclasses.replace(det, shift=shift, origin=shift - self._origin_offset(), strength=strength)
            rounds += 1
        self.relocation_history_ = np.array(history, dtype=np.float64).reshape(len(history), 3)
        return det, self.detection_gains(det)

    # -- detections relabelled: the alternatives under the other atoms and orientations ---------------------------------
    _OVER = ('transforms', 'atoms', 'all')

    def _alternative_set(self, over) -> Tuple[int, int]:
        """(n_alt, stride) of the candidate planes ``over`` names, with plane = atom * T + transform."""
        if not isinstance(over, str) or over not in self._OVER:
            raise ValueError(f'over must be one of {self._OVER}, not {over!r}')
        if over == 'transforms' and self._transforms is None:
            raise ValueError("over='transforms' needs a model with transforms")
        T = self.n_transforms
        return {'transforms': (T, 1), 'atoms': (self.n_atoms, T), 'all': (self.n_atoms * T, 1)}[over]

    def _alternatives(self, det, over, distinct: bool, who: str):
        """(a, b) ``[K, n_alt]`` float64 of the rows of ``det``, after the refusals and checks ``who`` shares with
        ``detection_gains``, (n_alt, stride), and the rows in the backend's terms."""
        self._plain_frobenius_only(who)
        rows = self._events_of(det, distinct=distinct)
        n_alt, stride = self._alternative_set(over)
        a, b = self._on_events('event_alternatives', events_alternatives_numpy, rows, n_alt, stride)
        return np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), (n_alt, stride), rows

    def detection_alternatives(self, det, over: str = 'transforms') -> Tuple[np.ndarray, np.ndarray]:
        """(a, b) float64: every row of ``det`` scored under other labels at its own shift, with everything else in the
        list held fixed -- ``over='transforms'`` the T orientations of the row's atom (``[K, T]``), ``'atoms'`` every atom in
        the row's orientation (``[K, M]``), ``'all'`` every atom and orientation (``[K, M, T]``).  With R =
        ``reconstruct_detections(det)`` and ``d = V - R + h phi`` the residual of the list without the row, ``a = <phi', d>``
        and ``b = ||phi'||^2`` for the candidate atom and orientation at the row's shift (phi': all its images, clipped to
        the sample).  The row relabelled so, at its best strength ``a / b``, would take ``a^2 / (2 b)`` off the objective of
        the list without the row (for ``a > 0``).  At the row's own label ``h (a - h b) + h^2 b / 2`` is its
        ``detection_gains`` and (a, b) are the centre of ``detection_landscape``.  Duplicate rows put back only themselves.
        On a backend with ``event_alternatives`` the list is rendered and scored on the device and only the ``2 K n_alt``
        numbers are copied.  The plain Frobenius objective only."""
        a, b, _, _ = self._alternatives(det, over, False, 'detection_alternatives')
        shape = (len(a), self.n_atoms, self.n_transforms) if over == 'all' else (len(a), a.shape[1])
        return a.reshape(shape), b.reshape(shape)

    def relabel_detections(self, det, over: str = 'transforms', n_iterations: int = 50, sparsity_H: float = 0.,
                           max_rounds: int = 100, min_improvement: float = 0., strengths: str = 'mu', tol: float = 1e-8,
                           max_iterations: int = 10000) -> Tuple[Detections, np.ndarray]:
        """Local search over the labels: the rows of ``det`` given the atom and orientation the data explains them better
        with, refitted, and their gains -- the fourth list operation beside ``pursue_detections`` (grow),
        ``prune_detections`` (shrink) and ``relocate_detections`` (move), and what it returns is what they return.  Each
        round refits the strengths (``refit_detections`` with ``n_iterations`` and ``sparsity_H``) and takes the alternatives
        (``detection_alternatives`` over ``over``).  For a row of strength h, with ``g = a^2 / (2 b)``, ``improvement = max
        over the other candidates of g - (h a_e + h^2 b_own / 2)``, ``a_e = a_own - h b_own``: what the objective falls by when
        the row takes its best other label at the strength ``a / b`` there.  The candidates are the rows with ``improvement >
        min_improvement`` whose best other label has ``g > 0``.  Per sample they are walked in descending improvement (ties in
        row order) and hop -- to the candidate of the lowest index among equal ones, ``shift`` and ``origin`` unchanged --
        unless the bounding box of the occurrence meets that of a hop already made in this round (rows with disjoint
        footprints do not interact, so their hops together are exact; the others are scored again next round), or the target
        is already a row of the list (the list stays distinct).  It stops when a round makes no hop or after ``max_rounds``
        rounds of hopping; ``max_rounds=0`` is a refit with its gains.  Read-out: ``relabel_history_`` ([rounds, 3]:
        candidates, hops, the sum of the hops' improvements).  The hops are chosen on the host; refit, render and
        alternatives run where the backend runs them.  The rows must be distinct; the plain Frobenius objective only.  With
        a process group every rank relabels the rows of its own samples: the call is not collective.  With
        ``strengths='solve'`` the strengths of every round are ``solve_detections(tol=, max_iterations=)``';
        ``n_iterations`` is unused and ``sparsity_H`` must be 0."""
        if self._plain_frobenius_only('relabel_detections'):
            self._alternative_set(over)   # (checked before the numbers; an unfitted model or a volume is refused first)
        _args.finite_number('min_improvement', min_improvement, '>= 0')
        _args.int_at_least('max_rounds', max_rounds, 0)
        T = self.n_transforms
        fitted = self._list_strengths('relabel_detections', strengths, n_iterations, sparsity_H, tol, max_iterations)
        history, rounds = [], 0
        while True:
            det = fitted(det)
            if rounds >= max_rounds:
                break
            a, b, (n_alt, stride), (sample, plane, shift, strength) = self._alternatives(det, over, True,
                                                                                         'relabel_detections')
            hopped, target, h, n_candidates, total = relabel_hops(
                sample, plane, shift, strength, a, b, n_alt, stride, self.atom_shape, self._V.shape[2:],
                tuple(int(x) for x in self._H.shape[2:]), self._mode, float(min_improvement))
            history.append((n_candidates, len(hopped), total))
            if not len(hopped):
                break
            atom, transform, strength = np.array(det.atom), np.array(det.transform), np.array(det.strength)
            atom[hopped], transform[hopped], strength[hopped] = target // T, target % T, h.astype(strength.dtype)
            det = dataclasses.replace(det, atom=atom, transform=transform, strength=strength)
            rounds += 1
        self.relabel_history_ = np.array(history, dtype=np.float64).reshape(len(history), 3)
        return det, self.detection_gains(det)

    def fit_detections(self, det, n_iterations: int = 50, sparsity_H: float = 0., update_H: bool = True,
                       update_W: bool = True) -> Detections:
        """Learn from the detections alone: ``n_iterations`` alternating multiplicative updates of the strengths
        (``update_H``: the step of ``refit_detections``) and of the dictionary (``update_W``: the W half step of a fit on
        activations that are zero off the support ``det``), against the model's own V -- templates refined from the events,
        without the sub-threshold activations ``detections()`` dropped.  Updates the model's ``W`` (and
        ``transformed_atoms``) in place and returns the rows with their refitted strengths.  An atom without evidence --
        no detections, only zero strengths, or only zero data under them -- keeps its entries.  The dense ``H`` is left
        as it is: ``R`` and ``objective()`` then describe the NEW W with the OLD dense H; what the detections explain is
        ``reconstruct_detections`` of the returned rows.  ``update_W=False`` is ``refit_detections``.  The rows must be
        distinct; the plain Frobenius objective only.  With a process group the call is collective: every rank calls with
        the detections of its own samples (possibly none) and the same ``n_iterations``."""
        _args.boolean('update_H', update_H)
        _args.boolean('update_W', update_W)
        if not update_H and not update_W:
            raise ValueError('fit_detections: update_H and update_W are both off')
        if not update_W:
            return self.refit_detections(det, n_iterations, sparsity_H)
        self._plain_frobenius_only('fit_detections')
        _args.int_at_least('n_iterations', n_iterations, 0)
        _args.finite_number('sparsity_H', sparsity_H, '>= 0')
        sample, plane, shift, strength = self._events_of(det, distinct=True)
        hook = getattr(self._backend, 'fit_events', None)
        if hook is not None:
            new = self._backend.to_ndarray(hook(self._V, self._W, self._W_eff, self._transforms, sample, plane, shift,
                                                strength, int(n_iterations), update_H=bool(update_H), update_W=True,
                                                sparsity=float(sparsity_H), eps=self.eps))
        else:
            W, *where = self._host_problem(self._W)
            W, new = events_fit_numpy(
                W, self._transforms, *where, sample, plane, shift, strength, self._local_V(), int(n_iterations),
                update_H=bool(update_H), update_W=True, sparsity=float(sparsity_H), eps=self.eps,
                normalize=lambda arr: self._backend.normalize(arr, axis=self._axes_W_normalization))
            self._W[...] = W
            self._expand_W()
        return self._with_strengths(det, shift, new)

    # -- the data under the detections, and how the occurrences of an atom vary ------------------------------------------
    def detection_patches(self, det, source: str = 'cleaned', frame: str = 'atom') -> np.ndarray:
        """``[K, C, *atom_shape]`` float64, in the order of ``det``: the data under each row -- the "waveforms" of the
        detections.  ``source``: ``'data'`` cuts V itself, ``'residual'`` ``V - R`` with R = ``reconstruct_detections(det)``,
        ``'cleaned'`` ``V - R + h phi``, the data with every OTHER row of the list taken out.  The cut is the adjoint of
        placing the atom: the signal under every image of the row (a wrapped or mirrored row has up to four) added up,
        pixels outside the sample contributing 0.  ``frame='image'`` leaves it in the frame of the transformed atom
        ``transformed_atoms[atom, transform]``; ``frame='atom'`` turns it back into the frame of ``W[atom]`` with the
        transposed operator of the row's transform (for a group: the inverse permutation), so that the patches of one atom
        align whatever their orientation and ``<W[atom], patch>`` is the row's correlation.  On a backend with
        ``event_patches`` the patches are gathered on the device and only they are copied.  The plain Frobenius objective
        only."""
        _args.one_of('source', source, _PATCH_SOURCES)
        _args.one_of('frame', frame, _PATCH_FRAMES)
        self._plain_frobenius_only('detection_patches')
        rows = self._events_of(det, distinct=False)
        out = self._on_events('event_patches', event_patches_numpy, rows, source=source, transforms=self._transforms,
                              frame=frame)
        return np.asarray(out, dtype=np.float64)

    def atom_patch_moments(self, det, source: str = 'cleaned', max_rows: Optional[int] = None):
        """(S ``[n_atoms, D, D]``, g ``[n_atoms, D]``, s2 ``[n_atoms]``, count ``[n_atoms]``) float64, ``D = C *
        prod(atom_shape)``: per atom the moments of the atom-frame patches y of its rows (``detection_patches(det, source)``
        flattened) and their strengths h: ``S = sum y y^T``, ``g = sum h y``, ``s2 = sum h^2``, ``count`` the rows.  All
        four are sums over the rows, so they add over disjoint lists -- and over the ranks of a process group: the call is
        not collective, each rank reports its own samples, as ``atom_terms`` does, and ``modes_from_moments`` takes the
        summed moments.  On a backend with ``event_patch_moments`` the patches never leave the device: the list is walked
        in chunks of at most ``max_rows`` rows (default: 256 MiB of patches), which does not change the result.  The plain
        Frobenius objective only."""
        _args.one_of('source', source, _PATCH_SOURCES)
        _args.int_at_least('max_rows', max_rows, 1, none_ok=True)
        self._plain_frobenius_only('atom_patch_moments')
        rows = self._events_of(det, distinct=False)
        out = self._on_events('event_patch_moments', event_patch_moments_numpy, rows, source=source,
                              transforms=self._transforms, max_rows=max_rows)
        return tuple(np.asarray(x, dtype=np.float64) for x in out)

    def atom_modes(self, det, n_modes: int = 3, source: str = 'cleaned'):
        """(mean ``[n_atoms, C, *A]``, modes ``[n_atoms, n_modes, C, *A]``, variance ``[n_atoms, n_modes]``, total
        ``[n_atoms]``) float64: how the occurrences of each atom vary -- the question opposite to ``atom_overlaps``, which
        two atoms are one: which one atom is two.  With y the atom-frame patches of an atom's rows and h their strengths,
        ``mean = sum h y / sum h^2`` is the least-squares template of the occurrences, and the modes are the leading
        eigenvectors of the scatter of ``y - h mean`` (``modes_from_moments``), unit vectors with the largest entry
        positive, ``variance`` their eigenvalues and ``total`` the trace: ``variance[m, 0] / total[m]`` near 1 says the
        occurrences of atom m differ along ONE direction -- the dictionary wants another atom, or another transform, there.
        An atom with fewer than two rows gets NaN modes and zero variance.  Leaves ``atom_modes_info_`` with the rows
        (``count``) and the summed squared strengths (``s2``) per atom.  Not collective (``atom_patch_moments``).  The plain
        Frobenius objective only."""
        _args.int_at_least('n_modes', n_modes, 1)
        if self._H is not None:   # (before the pass over the list; an unfitted model is refused by the helpers below)
            D = int(np.prod(self._W.shape[1:]))
            if n_modes > D:
                raise ValueError(f'n_modes must be an int in [1, {D}] (C * prod(atom_shape)), not {n_modes!r}')
        S, g, s2, count = self.atom_patch_moments(det, source)
        mean, modes, variance, total = modes_from_moments(S, g, s2, count, n_modes)
        shape = tuple(int(x) for x in self._W.shape[1:])
        self.atom_modes_info_ = dict(count=count, s2=s2)
        return mean.reshape((-1,) + shape), modes.reshape((len(mean), int(n_modes)) + shape), variance, total

    def sample_objective(self) -> np.ndarray:
        """[N] float64: each sample's share of ``objective()``, in the order of ``V`` (with a process group: this rank's
        samples, like ``H``).  Its sum is ``objective()``; for a fixed dictionary it is the anomaly score of a sample."""
        hook = getattr(self._backend, 'sample_objective', None)
        if hook is None:
            raise NotImplementedError(f'the backend {type(self._backend).__name__} has no per-sample objective')
        out = np.asarray(hook(self._V, self._W_dict, self._H, beta=self._beta, eps=self.eps), dtype=np.float64)
        return out if self._shuffle_idx is None else out[np.argsort(self._shuffle_idx)]

    def atom_terms(self) -> Tuple[np.ndarray, np.ndarray]:
        """(a, b), float64 ``[N, n_atoms]``: with ``R_m`` the contribution of atom m (in all its orientations, as
        ``R_partial(m)``) and ``d = V - R``, ``a[n, m] = <R_m[n], d[n]>`` and ``b[n, m] = ||R_m[n]||^2`` -- after a weighted
        fit ``sum G R_m d`` and ``sum G R_m^2``.  Without atom m the objective of sample n rises by ``a + b / 2``
        (``atom_gains``); ``1 + a / b`` is the factor that rescales the atom's activations in that sample best, a
        diagnostic after a fit under ``sparsity_H``.  Samples in the order of ``H`` (with a process group: this rank's
        samples, and the call is not collective).  On a backend with ``atom_terms`` one pass over the activations where they
        live; any other backend's are scored on the host.  The Frobenius objective only; ``W``, ``H`` and ``V`` are not
        touched."""
        self._atom_refusals()
        hook = getattr(self._backend, 'atom_terms', None)
        if hook is not None:
            a, b = hook(self._V, self._W_dict, self._H, self.n_transforms)
        else:
            G = self._weights
            if G is not None and len(G) != int(self._H.shape[0]):
                n0 = int(getattr(self._backend, 'shard', (0, 0))[0])
                G = G[n0:n0 + int(self._H.shape[0])]
            a, b = atom_terms_numpy(self._backend.to_ndarray(self._W_dict), self._backend.to_ndarray(self._H),
                                    self._mode, self._local_V(), G, self.n_transforms)
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        if self._shuffle_idx is not None:
            order = np.argsort(self._shuffle_idx)
            a, b = a[order], b[order]
        return a, b

    def atom_gains(self, per_sample: bool = False) -> np.ndarray:
        """What each atom explains: the objective of the model without atom m (in all its orientations) minus that of the
        model, ``1/2 ||V - (R - R_m)||^2 - 1/2 ||V - R||^2 = a + b / 2`` with the terms of ``atom_terms`` -- in the unit of
        ``detection_gains``, so an atom and a detection compare.  ``[n_atoms]`` float64, summed over the samples, or with
        ``per_sample=True`` ``[N, n_atoms]`` in the order of ``H``.  Not collective: with a process group each rank reports
        its own samples and the sum over the ranks is the caller's, as for ``detection_errors``.  The Frobenius objective,
        with or without weights."""
        _args.boolean('per_sample', per_sample)
        a, b = self.atom_terms()
        gain = a + 0.5 * b
        return gain if per_sample else gain.sum(axis=0)

    # -- the sources of a sample: per-source signals by soft masks ---------------------------------------------------------
    def _source_tables(self, sources) -> Tuple[np.ndarray, np.ndarray]:
        """The refusals of ``separate`` and the two int32 tables of its sources: the planes, source after source (an atom
        stands for its ``n_transforms`` planes), and where each source starts."""
        if sources is None:
            sets = [[m] for m in range(self.n_atoms)]
        else:
            sets = _args.disjoint_index_sets('sources', sources, self.n_atoms)
        if self._H is None:
            raise RuntimeError('the sources of a model need a fitted model: call fit first')
        if len(self.atom_shape) == 3:
            raise NotImplementedError('separate: 1 or 2 shift axes only')
        return source_tables(sets, self.n_transforms)

    def _in_order_of_V(self, out: np.ndarray) -> np.ndarray:
        return out if self._shuffle_idx is None else out[np.argsort(self._shuffle_idx)]

    def separate(self, sources=None, output: str = 'masked') -> np.ndarray:
        """The sample split into its sources, ``[N, S, C, *D]`` in V's dtype.  ``sources``: a sequence of S disjoint,
        non-empty sequences of atom indices (with ``transforms`` an atom stands for all its orientations); ``None``: every
        atom is a source of its own.  With ``r_g`` the sum of what the atoms of source g add to R and ``total`` the sum over
        ALL atoms -- atoms in no source count there and get no output -- ``output`` selects

        * ``'contribution'``: ``r_g``, the source's part of R;
        * ``'mask'``: ``r_g / (total + eps)``, the soft (Wiener-type) mask, in [0, 1];
        * ``'masked'``: ``V * (r_g / (total + eps))``, the source's estimate, in [0, V]; over a partition of the atoms the
          estimates add up to ``V * R / (R + eps)``, whatever objective was fitted

        with the model's ``eps``; 0 where ``total + eps`` is 0.  Weights play no part in the arithmetic: the V of a weighted
        fit holds 0 where the weight is 0, so ``'masked'`` is 0 there, while ``'contribution'`` is the model's imputation of
        the hidden entries.  Samples in the order of ``V`` (with a process group: this rank's samples, and the call is not
        collective).  On a backend with ``source_parts`` one pass over the activations where they live, every denominator
        that pass's own sum; any other backend's sources are separated on the host in float64.  Any ``beta_loss``, 1 or 2
        shift axes; ``W``, ``H`` and ``V`` are not touched."""
        _args.one_of('output', output, _SOURCE_OUTPUTS)
        order, start = self._source_tables(sources)
        out = None
        if getattr(self._backend, 'supports_sources', False):
            try:
                out = self._backend.to_ndarray(self._backend.source_parts(self._V, self._W_dict, self._H, order, start,
                                                                          output, eps=self.eps))
            except NotImplementedError:   # (a tile of H beyond the kernel's LDS: nothing was written)
                out = None
        if out is None:
            V, G = self._local_V(), self._weights
            if G is not None:   # (entries of weight 0 are not data: they count as 0, as on a backend that binds the weights)
                if len(G) != len(V):
                    n0 = int(getattr(self._backend, 'shard', (0, 0))[0])
                    G = G[n0:n0 + len(V)]
                V = np.where(G > 0, V, 0)
            out = separate_numpy(self._backend.to_ndarray(self._W_dict), self._backend.to_ndarray(self._H), self._mode,
                                 V, order, start, output, self.eps)
        return self._in_order_of_V(np.asarray(out).astype(self._V.dtype, copy=False))

    def dominant_source(self, sources=None) -> Tuple[np.ndarray, np.ndarray]:
        """A segmentation of the samples by source: ``(label, share)``, both ``[N, *D]``.  ``label`` (int32) is the index g
        of the source -- ``sources`` as for ``separate`` -- with the largest contribution summed over the channels,
        ``sum_c r_g``, at the pixel; the lowest index wins a tie, and where the model explains nothing (``sum_c total == 0``)
        the label is -1.  ``share`` (V's dtype) is that sum over ``sum_c total + eps``.  Samples in the order of ``V``; not
        collective."""
        order, start = self._source_tables(sources)
        out = None
        if getattr(self._backend, 'supports_sources', False):
            try:
                label, share = self._backend.dominant_parts(self._V, self._W_dict, self._H, order, start, eps=self.eps)
                out = self._backend.to_ndarray(label), self._backend.to_ndarray(share)
            except NotImplementedError:
                out = None
        if out is None:
            out = dominant_numpy(self._backend.to_ndarray(self._W_dict), self._backend.to_ndarray(self._H), self._mode,
                                 self._V.shape[2:], order, start, self.eps)
        label, share = out
        return (self._in_order_of_V(np.asarray(label).astype(np.int32, copy=False)),
                self._in_order_of_V(np.asarray(share).astype(self._V.dtype, copy=False)))

    # -- which atoms co-occur, and at what offset: the correlogram of the activations ------------------------------------
    def _max_lag(self, max_lag) -> Tuple[int, ...]:
        """``max_lag`` as one int >= 0 per shift axis; ``None``: ``atom_shape - 1``, the range over which two occurrences
        touch."""
        k = len(self.atom_shape)
        if max_lag is None:
            return tuple(int(a) - 1 for a in self.atom_shape)
        if _args.is_int(max_lag):
            lags = (max_lag,) * k
        elif isinstance(max_lag, (tuple, list)) and len(max_lag) == k:
            lags = tuple(max_lag)
        else:
            raise ValueError(f'max_lag must be None, an int or {k} ints, not {max_lag!r}')
        for lag in lags:
            _args.int_at_least('max_lag', lag, 0)
        return tuple(int(lag) for lag in lags)

    def activation_correlogram(self, max_lag: Union[None, int, Tuple[int, ...]] = None,
                               per_sample: bool = False) -> np.ndarray:
        """How often plane q fires at offset D from plane p: ``C[p, q, D] = sum_n sum_u H[n, p, u] H[n, q, u + D]`` over
        the u with u and u + D inside the plane (nothing wraps, in any reconstruction mode), for the lags
        ``|D_k| <= max_lag[k]`` with lag ``D_k`` at index ``D_k + max_lag[k]``: float64 ``[P, P, *(2 L + 1)]``, or with
        ``per_sample=True`` ``[N, P, P, *(2 L + 1)]`` in the order of ``H``.  P counts the effective planes (``atom * T +
        transform`` with transforms).  ``C[p, q, D] == C[q, p, -D]``, and ``C[p, q, D]^2 <= C[p, p, 0] C[q, q, 0]``.

        max_lag : ``None`` (``atom_shape - 1``: the range over which two occurrences touch), an int or one int >= 0 per
                  shift axis; lags at or beyond the extent of an axis are 0

        The correlogram reads ``H`` alone: any ``beta_loss``, weights, reconstruction mode and transforms.  On a backend
        with ``activation_correlogram`` one pass over the activations where they live, every sum in double; any other
        backend's ``H`` -- and a lag beyond that hook's limit -- goes through ``activation_correlogram_numpy`` on the
        host.  Not collective: with a process group each rank reports its own samples, and C adds over the ranks."""
        if self._H is None:
            raise RuntimeError('activation_correlogram() needs a fitted model: call fit first')
        lags = self._max_lag(max_lag)
        _args.boolean('per_sample', per_sample)
        hook = getattr(self._backend, 'activation_correlogram', None)
        C = None
        if hook is not None:
            try:
                C = hook(self._H, lags, per_sample=bool(per_sample))
            except NotImplementedError:   # (volumes, a lag beyond the kernel's limit: nothing was written)
                C = None
        if C is None:
            C = activation_correlogram_numpy(self._backend.to_ndarray(self._H), lags, bool(per_sample))
        C = np.asarray(C, dtype=np.float64)
        return self._in_order_of_V(C) if per_sample else C

    def atom_cooccurrence(self, max_lag: Union[None, int, Tuple[int, ...]] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(score ``[P, P]`` float64, lag ``[P, P, k]`` int64): ``score[p, q] = max_D C[p, q, D] / sqrt(C[p, p, 0]
        C[q, q, 0])`` of ``activation_correlogram(max_lag)``, in [0, 1], and ``lag`` the D that reaches it (the first in C
        order on a tie).  For p == q the lag 0 is left out; a plane with ``C[p, p, 0] == 0`` scores 0.  A score near 1 at
        ``lag != 0`` says q is p's fixed-offset partner -- two halves of one larger motif: the atom window is too small, or
        ``n_atoms`` too large; a high ``score[p, p]`` at lag D is a rhythm of period D.  Host algebra on the one pass; not
        collective."""
        return cooccurrence(self.activation_correlogram(max_lag))

    # -- the data around the places where an atom fires: triggered sums on a window larger than the atom ----------------
    def _margin(self, margin) -> Tuple[int, ...]:
        """``margin`` as one int >= 0 per shift axis; ``None``: ``(a + 1) // 2``, a window about twice the atom."""
        k = len(self.atom_shape)
        if margin is None:
            return tuple((int(a) + 1) // 2 for a in self.atom_shape)
        if _args.is_int(margin):
            margins = (margin,) * k
        elif isinstance(margin, (tuple, list)) and len(margin) == k:
            margins = tuple(margin)
        else:
            raise ValueError(f'margin must be None, an int or {k} ints, not {margin!r}')
        for x in margins:
            _args.int_at_least('margin', x, 0)
        return tuple(int(x) for x in margins)

    def _triggered_refusals(self, what: str) -> None:
        if self._H is None:
            raise RuntimeError(f'{what}() needs a fitted model: call fit first')
        if len(self.atom_shape) == 3:
            raise NotImplementedError(f'{what}: 1 or 2 shift axes only')

    def _triggered(self, source: str, margin: Tuple[int, ...], power: int = 1, per_sample: bool = False) -> np.ndarray:
        """The triggered sums of the field ``source`` ('data', 'reconstruction', 'residual', each times the weights of a
        weighted fit, or 'weights': the weights, ones without), float64, samples in the order of ``H``."""
        backend = self._backend
        if getattr(backend, 'supports_triggered', False):
            Y = backend.triggered_field(self._V, self._W_dict, self._H, source)
            try:
                return np.asarray(backend.triggered_sums(self._H, Y, margin, power=power, per_sample=per_sample),
                                  dtype=np.float64)
            except NotImplementedError:   # (a window beyond the kernel's limit: nothing was written)
                Y = backend.to_ndarray(Y)
        else:
            V, G = np.asarray(self._local_V(), dtype=np.float64), self._weights
            if G is not None and len(G) != len(V):
                n0 = int(getattr(backend, 'shard', (0, 0))[0])
                G = G[n0:n0 + len(V)]
            if source == 'weights':
                Y = np.ones(V.shape) if G is None else np.where(G > 0, G, 0.)
            else:
                R = None if source == 'data' else np.asarray(backend.to_ndarray(backend.reconstruct(self._W_dict, self._H)),
                                                             dtype=np.float64)
                Y = V if source == 'data' else R if source == 'reconstruction' else V - R
                if G is not None:   # (entries of weight 0 are not data: they add exactly 0 whatever V holds there)
                    with np.errstate(invalid='ignore'):
                        Y = np.where(G > 0, G * Y, 0.)
        Hp = pad_activations_numpy(backend.to_ndarray(self._H), self.atom_shape, self._mode)
        return triggered_sums_numpy(Hp, Y, self.atom_shape, margin, power, per_sample)

    def activation_triggered_sums(self, margin: Union[None, int, Tuple[int, ...]] = None, source: str = 'residual',
                                  per_sample: bool = False) -> np.ndarray:
        """The data around the places where a plane fires: ``X[p, c, j] = sum_n sum_q Hp[n, p, q] S[n, c, q - (A - 1) - m
        + j]`` for ``0 <= j_k < A_k + 2 m_k``, with ``Hp`` the padded activations every mode reconstructs from and ``S`` the
        field ``source`` of the samples' shape; terms whose index falls outside the sample are absent.  float64
        ``[P, C, *(A + 2 m)]``, or with ``per_sample=True`` ``[N, P, C, *(A + 2 m)]`` in the order of ``V``.  P counts the
        effective planes (``atom * T + transform`` with transforms).

        margin : ``None`` (``(a + 1) // 2`` per axis: a window about twice the atom), an int or one int >= 0 per shift axis
        source : ``'data'`` (V), ``'reconstruction'`` (R) or ``'residual'`` (V - R); after a weighted fit each is
                 multiplied by the weights

        The entries ``[m, m + A)`` of the window are ``neg`` (data) and ``pos`` (reconstruction) of the W gradient of the
        effective planes -- of the Frobenius objective only; under any other ``beta_loss`` the sums are a plain correlation
        and no gradient.  The entries outside are what that gradient would be for taps the atom does not have.  Any
        ``beta_loss``, weights, reconstruction mode and transforms; 1 or 2 shift axes.  On a backend with
        ``triggered_sums`` one pass over the activations where they live, every sum in double; any other backend -- and a
        window beyond that hook's limit -- goes through ``triggered_sums_numpy`` on the host.  Not collective: with a
        process group each rank reports its own samples, and X adds over the ranks.  ``W``, ``H`` and ``V`` are not
        touched."""
        self._triggered_refusals('activation_triggered_sums')
        m = self._margin(margin)
        _args.one_of('source', source, _TRIGGERED_SOURCES)
        _args.boolean('per_sample', per_sample)
        X = self._triggered(source, m, 1, bool(per_sample))
        return self._in_order_of_V(X) if per_sample else X

    def activation_triggered_average(self, margin: Union[None, int, Tuple[int, ...]] = None,
                                     source: str = 'data') -> np.ndarray:
        """The weighted mean of the field's values where plane p fires -- the spike-triggered average of the dense model:
        ``activation_triggered_sums(margin, source)`` divided by ``mass[p, c, j] = sum Hp G`` over the same terms (G the
        weights of a weighted fit, else 1), float64 ``[P, C, *(A + 2 m)]``; NaN where ``mass == 0``.  Arguments and limits
        as for ``activation_triggered_sums``."""
        self._triggered_refusals('activation_triggered_average')
        m = self._margin(margin)
        _args.one_of('source', source, _TRIGGERED_SOURCES)
        X, mass = self._triggered(source, m), self._triggered('weights', m)
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(mass == 0, np.nan, X / mass)

    def atom_tap_gains(self, margin: Union[None, int, Tuple[int, ...]] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(gain, step), float64 ``[P, C, *(A + 2 m)]``: would a larger ``atom_shape`` pay, on which side, for which atom.
        With ``E`` the triggered sums of ``G (V - R)`` and ``b = sum Hp^2 G`` over the same terms, the objective as a
        function of a change t of ONE tap of ONE effective plane, everything else held, is ``-t E + t^2 b / 2``; a tap stays
        >= 0, so ``step = max(E / b, -W_ext)`` (``W_ext`` the effective atoms zero-extended to the window; 0 where ``b`` is
        0) and ``gain = step E - step^2 b / 2 >= 0`` is the exact drop of ``1/2 ||V - R||^2`` (weighted when weights are
        bound) under that one change -- the ``a^2 / (2 b)`` of ``pursue_detections``.  Entries outside ``[m, m + A)`` are
        taps the atom does not have.

        What this is not: taps interact through the autocorrelogram of H, so the gains of several taps do not add; with
        ``transforms`` the planes of an atom share their taps; and W is normalised after every step.  Sums of gains rank
        atoms and sides of the window; they do not predict the objective of a refit.

        The Frobenius objective only, with or without weights; 1 or 2 shift axes; not collective; ``W``, ``H`` and ``V`` are
        not touched."""
        self._atom_refusals()
        m = self._margin(margin)
        E, b = self._triggered('residual', m), self._triggered('weights', m, power=2)
        W_ext = extend_atoms(self._backend.to_ndarray(self._W_dict), m)
        return tap_gains_from_sums(E, b, W_ext)

    def atom_window_gains(self, margin: Union[None, int, Tuple[int, ...]] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(inside, outside), float64 ``[n_atoms]``: the gains of ``atom_tap_gains(margin)`` summed over an atom's planes,
        its channels and the taps inside / outside ``[m, m + A)``.  An ``outside`` that is not small beside ``inside`` says
        this atom wants a larger ``atom_shape``; the per-tap map says on which side.  A ranking, not a prediction."""
        gain, _ = self.atom_tap_gains(margin)
        return window_gains(gain, self._margin(margin), self.n_atoms)

    # -- how atoms overlap: a and the Gram matrix B of the atoms' contributions ------------------------------------------
    # With per-atom scale factors s (R(s) = sum s_m R_m) the objective is the exact quadratic
    #   E(s) = E(1) - a^T (s - 1) + 1/2 (s - 1)^T B (s - 1),        B[m, m'] = sum G R_m R_m'  (diag(B) = b of atom_terms)
    # so after ONE pass over H everything below is host algebra on an [n_atoms, n_atoms] matrix.
    def _atom_refusals(self) -> None:
        """What ``atom_terms`` refuses, with its messages."""
        if self._H is None:
            raise RuntimeError('the atom gains of a model need a fitted model: call fit first')
        if self._beta != 2.:
            raise NotImplementedError('atom_gains covers the Frobenius objective (beta_loss 2), with or without weights')
        if len(self.atom_shape) == 3:
            raise NotImplementedError('atom gains: 1 or 2 shift axes only')

    def _atom_gram(self) -> Tuple[np.ndarray, np.ndarray]:
        """(a [N, n_atoms], B [N, n_atoms, n_atoms]), float64, samples in the order of ``H``; refuses what ``atom_terms``
        refuses."""
        self._atom_refusals()
        hook = getattr(self._backend, 'atom_gram', None)
        if hook is not None:
            a, B = hook(self._V, self._W_dict, self._H, self.n_transforms)
        else:
            G = self._weights
            if G is not None and len(G) != int(self._H.shape[0]):
                n0 = int(getattr(self._backend, 'shard', (0, 0))[0])
                G = G[n0:n0 + int(self._H.shape[0])]
            a, B = atom_gram_numpy(self._backend.to_ndarray(self._W_dict), self._backend.to_ndarray(self._H),
                                   self._mode, self._local_V(), G, self.n_transforms)
        a, B = np.asarray(a, dtype=np.float64), np.asarray(B, dtype=np.float64)
        if self._shuffle_idx is not None:
            order = np.argsort(self._shuffle_idx)
            a, B = a[order], B[order]
        return a, B

    def atom_gram(self, per_sample: bool = False) -> np.ndarray:
        """``B[m, m'] = <R_m, R_m'>`` (after a weighted fit ``sum G R_m R_m'``) with ``R_m`` the contribution of atom m in
        all its orientations: float64 ``[n_atoms, n_atoms]`` summed over the samples, or with ``per_sample=True``
        ``[N, n_atoms, n_atoms]`` in the order of ``H``.  Symmetric; its diagonal is ``b`` of ``atom_terms``.  On a backend
        with ``atom_gram`` one pass over the activations where they live.  Not collective: with a process group each rank
        reports its own samples.  The Frobenius objective, with or without weights; ``W``, ``H``, ``V`` are not touched."""
        _args.boolean('per_sample', per_sample)
        B = self._atom_gram()[1]
        return B if per_sample else B.sum(axis=0)

    # -- the same questions under the model's own objective, any beta_loss ------------------------------------------------
    # With x = max(R, 0) + eps, x_m = max(R - R_m, 0) + eps and D the element divergence of the objective:
    #   gain = sum G (D(V | x_m) - D(V | x))                                  exact: the objective without atom m, minus the objective
    #   a = sum G R_m (V x^(beta-2) - x^(beta-1)),   B = sum G c R_m R_m',    c = (beta-1) x^(beta-2) + (2-beta) V x^(beta-3)
    # E(s) ~ E(1) - a^T (s - 1) + 1/2 (s - 1)^T B (s - 1) is the local second-order model in per-atom scale factors, exact
    # only at beta_loss 2, where all of this is atom_terms / atom_gains / atom_gram.
    def _atom_divergence(self, gram: bool):
        """(a, b, gain) or (a, B), float64, samples in the order of ``H``: the backend's hook, else the host fallback."""
        if self._H is None:
            raise RuntimeError('the atom gains of a model need a fitted model: call fit first')
        if len(self.atom_shape) == 3:
            raise NotImplementedError('atom gains: 1 or 2 shift axes only')
        if self._beta == 2.:
            if gram:
                return self._atom_gram()
            a, b = self.atom_terms()
            return a, b, a + 0.5 * b
        name = 'atom_divergence_gram' if gram else 'atom_divergence_terms'
        hook = getattr(self._backend, name, None)
        if hook is not None:
            out = hook(self._V, self._W_dict, self._H, self.n_transforms, self._beta, self.eps)
        else:
            G = self._weights
            if G is not None and len(G) != int(self._H.shape[0]):
                n0 = int(getattr(self._backend, 'shard', (0, 0))[0])
                G = G[n0:n0 + int(self._H.shape[0])]
            fallback = atom_divergence_gram_numpy if gram else atom_divergence_terms_numpy
            out = fallback(self._backend.to_ndarray(self._W_dict), self._backend.to_ndarray(self._H), self._mode,
                           self._local_V(), G, self.n_transforms, self._beta, self.eps)
        out = tuple(np.asarray(o, dtype=np.float64) for o in out)
        if self._shuffle_idx is not None:
            order = np.argsort(self._shuffle_idx)
            out = tuple(o[order] for o in out)
        return out

    def atom_divergence_terms(self) -> Tuple[np.ndarray, np.ndarray]:
        """(a, b), float64 ``[N, n_atoms]``, under the model's own objective (any ``beta_loss``, with or without weights):
        with ``R_m`` the contribution of atom m in all its orientations and ``x = max(R, 0) + eps``,
        ``a = sum G R_m (V x^(beta-2) - x^(beta-1))`` is minus the slope and ``b = sum G R_m^2 c``,
        ``c = (beta-1) x^(beta-2) + (2-beta) V x^(beta-3)``, the curvature of sample n's objective in a scale factor on atom
        m, at 1.  A local model, not an identity: ``1 + a / b`` is one Newton step towards the best rescaling of the atom,
        and ``b`` can be negative for ``beta_loss`` outside [1, 2].  What IS exact is ``atom_divergence_gains``.  Samples in
        the order of ``H``; not collective; one pass over the activations on a backend with the hook, the host otherwise.
        At ``beta_loss`` 2 this is ``atom_terms``.  ``W``, ``H`` and ``V`` are not touched."""
        return self._atom_divergence(False)[:2]

    def atom_divergence_gains(self, per_sample: bool = False) -> np.ndarray:
        """What each atom explains under the model's own objective: ``sample_objective()`` of the model without atom m (in
        all its orientations; its planes of ``H`` at 0) minus ``sample_objective()`` of the model -- exact, for any
        ``beta_loss``, with or without weights, in one pass over the activations.  ``[n_atoms]`` float64, summed over the
        samples, or with ``per_sample=True`` ``[N, n_atoms]`` in the order of ``H``.  Not collective.  Where an atom alone
        explains a pixel with ``V > 0`` the model without it falls to ``eps`` there and the gain carries a term of the size
        ``V log(R / eps)`` (Kullback-Leibler; ``V / eps`` for Itakura-Saito): that is the objective's own, not an artefact.
        At ``beta_loss`` 2 this is ``atom_gains``."""
        _args.boolean('per_sample', per_sample)
        gain = self._atom_divergence(False)[2]
        return gain if per_sample else gain.sum(axis=0)

    def atom_divergence_gram(self, per_sample: bool = False) -> np.ndarray:
        """``B[m, m'] = sum G c R_m R_m'`` with the curvature weights ``c`` of ``atom_divergence_terms``: the Hessian of the
        objective in per-atom scale factors at 1, float64 ``[n_atoms, n_atoms]`` summed over the samples, or with
        ``per_sample=True`` ``[N, n_atoms, n_atoms]`` in the order of ``H``.  Symmetric; its diagonal is ``b``.  With ``a``,
        ``E(s) ~ E(1) - a^T (s - 1) + 1/2 (s - 1)^T B (s - 1)`` is a local model, exact only at ``beta_loss`` 2 (where this is
        ``atom_gram``); for ``beta_loss`` outside [1, 2] the weights are signed and ``B`` need not be positive
        semi-definite.  Not collective; ``W``, ``H``, ``V`` are not touched."""
        _args.boolean('per_sample', per_sample)
        B = self._atom_divergence(True)[1]
        return B if per_sample else B.sum(axis=0)

    def atom_overlaps(self) -> np.ndarray:
        """``B[m, m'] / sqrt(B[m, m] B[m', m'])``, float64 ``[n_atoms, n_atoms]``: the cosine between two atoms'
        contributions to R, 1 for duplicates -- duplicates up to a shift included, since H absorbs the shift -- and 0 where
        an atom is dead (contributes nothing)."""
        B = self._atom_gram()[1].sum(axis=0)
        norm = np.sqrt(np.diag(B))
        live = norm > 0
        out = np.zeros_like(B)
        out[np.ix_(live, live)] = B[np.ix_(live, live)] / np.outer(norm[live], norm[live])
        out[live, live] = 1.
        return out

    def _atom_indices(self, atoms) -> np.ndarray:
        try:
            items = list(atoms)
        except TypeError:
            raise ValueError(f'atoms must be a sequence of distinct ints in [0, {self.n_atoms}), not {atoms!r}') from None
        for m in items:
            if not _args.is_int(m) or not 0 <= m < self.n_atoms:
                raise ValueError(f'atoms must be distinct ints in [0, {self.n_atoms}), not {m!r}')
        if len(set(int(m) for m in items)) != len(items):
            raise ValueError(f'atoms must be distinct: {items!r}')
        return np.asarray(items, dtype=np.int64)

    def atom_set_gain(self, atoms) -> float:
        """What the atoms in ``atoms`` explain together: the exact rise of the objective without them (their activations
        set to zero, everything else held), ``sum_S a + 1/2 sum_SS B``.  A single atom gives ``atom_gains()[m]``.
        ``atoms``: distinct ints in ``[0, n_atoms)``."""
        idx = self._atom_indices(atoms)
        a, B = self._atom_gram()
        return gram_set_gain(a.sum(axis=0), B.sum(axis=0), idx)

    def atom_scales(self, nonnegative: bool = True) -> np.ndarray:
        """The per-atom scale factors ``s`` of the activations, ``[n_atoms]`` float64, that fit V best with everything else
        held: the minimiser of ``E(s)``, ``B s = a + B 1``, over ``s >= 0`` unless ``nonnegative=False`` (an active-set
        solve on the host) -- after a fit under ``sparsity_H``, the shrinkage undone for all atoms at once.  Dead atoms get
        scale 1; a singular block, such as two exact duplicates, its minimum-norm solution."""
        _args.boolean('nonnegative', nonnegative)
        a, B = self._atom_gram()
        return gram_scales(a.sum(axis=0), B.sum(axis=0), bool(nonnegative))

    def rescale_atoms(self, scales=None) -> float:
        """Multiply the activations of atom m (all its orientations) by ``scales[m]`` in place -- ``None``:
        ``atom_scales()`` -- and return the predicted drop of the objective, ``a^T (s - 1) - 1/2 (s - 1)^T B (s - 1)``
        (exact for the Frobenius objective up to rounding).  Leaves the factors in ``atom_scales_``.  ``scales``:
        ``[n_atoms]`` finite numbers >= 0.  With a process group ``scales`` must be given: the (a, B) of this call are this
        rank's, and a global ``s`` is the caller's all-reduce of ``atom_terms`` / ``atom_gram``."""
        if scales is not None:
            s = np.asarray(scales, dtype=np.float64)
            if s.shape != (self.n_atoms,) or not np.all(np.isfinite(s)) or np.any(s < 0):
                raise ValueError(f'scales must be {self.n_atoms} finite numbers >= 0, not {scales!r}')
        self._atom_refusals()
        if scales is None and int(getattr(self._backend, '_world', 1)) > 1:   # (before the pass over H)
            raise NotImplementedError('rescale_atoms with a process group needs the scales: reduce atom_terms and '
                                      'atom_gram over the ranks and pass the global scales')
        a, B = self._atom_gram()
        a, B = a.sum(axis=0), B.sum(axis=0)
        if scales is None:
            s = gram_scales(a, B, True)
        drop = gram_drop(a, B, s)
        T = self.n_transforms
        for m in np.flatnonzero(s != 1.):
            self._H[:, m * T:(m + 1) * T] *= float(s[m])   # (in place: an array library's own operation, which its caches see)
        self.atom_scales_ = s
        return drop

    def atom_elimination(self, rescale: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Backward elimination of atoms on ``(a, B)`` alone -> ``(order, rise)``: ``order[k]`` is the atom whose removal
        raises the objective least given ``order[:k]`` already removed, ``rise[k]`` the cumulative rise of the objective
        over the model as it stands once ``order[:k + 1]`` are gone.  ``rescale=True``: the remaining atoms are rescaled
        optimally (``s >= 0``) at every step, so ``rise`` may begin below zero.  One pass over H, then host algebra; the
        model is not touched."""
        _args.boolean('rescale', rescale)
        a, B = self._atom_gram()
        return gram_elimination(a.sum(axis=0), B.sum(axis=0), bool(rescale))

    # -- stopping on the objective ---------------------------------------------------------------------------------
    @staticmethod
    def _convergence_args(objective_every, tol) -> Tuple[Optional[int], Optional[float]]:
        """(objective_every, tol) checked; ``tol`` alone records every 10 iterations (scikit-learn's cadence)."""
        # (a number is converted before its range is checked: the message shows the plain float or int)
        if tol is not None:
            tol = float(tol) if _args.is_real(tol) else tol
            _args.finite_number('tol', tol, '>= 0')
            if objective_every is None:
                objective_every = 10
        if objective_every is not None:
            objective_every = int(objective_every) if _args.is_int(objective_every) else objective_every
            _args.int_at_least('objective_every', objective_every, 1)
        return objective_every, tol

    def _begin_history(self) -> None:
        self._history = []
        self.objective_history_ = np.empty((0, 2))
        self.n_iter_ = 0
        self.converged_ = False
        self._objective_buf = None

    def _record(self, step: int, value: float, tol: Optional[float]) -> bool:
        """Note the objective ``value`` of the state that entered ``step``; True when the fit ends with this step."""
        self._history.append((step, value))
        if not math.isfinite(value):
            warnings.warn(f'the objective is {value} at step {step}: the fit stops', RuntimeWarning, stacklevel=3)
            return True
        if tol is not None and len(self._history) >= 2:
            if self._history[-2][1] - value <= tol * self._history[0][1]:
                self.converged_ = True
                return True
        return False

    def _end_history(self, n_iter: int) -> None:
        self.n_iter_ = n_iter
        self.objective_history_ = np.asarray(self._history, dtype=np.float64).reshape(-1, 2)
        self._objective_buf = None

    # -- elementwise multiplicative update (reference :217-238) ----------------------------------------------
    def _multiplicative_update(self, arr, neg, pos, sparsity: float = 0., normalization_axes=None):
        assert sparsity >= 0
        regularization = self.eps + (sparsity if sparsity > 0 else 0.)
        hook = getattr(self._backend, 'multiplicative_update', None)
        if hook is not None:
            hook(arr, neg, pos, regularization)
        else:
            pos += regularization
            arr *= neg
            arr /= pos
        if normalization_axes is not None:
            self._backend.normalize(arr, axis=normalization_axes)

    # -- half steps (reference :240-271) ----------------------------------------------------------------------
    def _fused(self, name: str):
        return getattr(self._backend, name, None) if self._use_fused else None

    def _step_hook(self, name: str):
        """_fused(name); any objective but the plain Frobenius one always takes the backend's hook (the reference's
        Frobenius lines do not apply to it)."""
        return getattr(self._backend, name) if not self._plain_frobenius else self._fused(name)

    def _update_W(self, s: slice = sliceNone):
        if self._transforms is not None:
            # gradient of W_eff, folded onto W (before any collective), MU + normalise, expanded again
            self._backend.fused_update_W_transformed(self._V, self._W, self._W_eff, self._H, s, self._transforms,
                                                     **self._objective(eps=self.eps))
            return
        fused = self._step_hook('fused_update_W')
        if fused is not None:
            fused(self._V, self._W, self._H, s, **self._objective(eps=self.eps))
            return
        neg, pos = self._backend.reconstruction_gradient_W(self._V, self._W, self._H, s)
        assert neg.shape == self._W.shape and pos.shape == self._W.shape
        self._multiplicative_update(self._W, neg, pos, normalization_axes=self._axes_W_normalization)

    def _update_H(self, s: slice = sliceNone, sparsity: float = 0., inhibition: float = 0., cross_inhibition: float = 0.,
                  record: bool = False) -> Optional[float]:
        """record: this step is to yield the objective of the state it starts from.  Returns None when the backend's H half
        step taps it (into self._objective_buf, read later), else its value, evaluated before anything is written."""
        lateral = inhibition > 0 or cross_inhibition > 0
        fused = self._step_hook('fused_update_H')
        tap = record and fused is not None and getattr(self._backend, 'supports_objective_tap', False)
        value = self._energy_function() if record and not tap else None
        if fused is not None:
            kw = dict(inhibition=inhibition, cross_inhibition=cross_inhibition,
                      inhibition_kernels=self._inhibition_kernels_1D) if lateral else {}
            if tap:   # (the keyword is passed only when the step records)
                if self._objective_buf is None:
                    self._objective_buf = self._backend.new_objective_buffer()
                kw['objective_out'] = self._objective_buf
            try:
                fused(self._V, self._W_dict, self._H, s, sparsity=sparsity, **self._objective(eps=self.eps, **kw))
                return value
            except NotImplementedError:
                # (inhibition kernels longer than the backend's fused kernel takes; lateral terms or reconstruction modes
                # of volumes: nothing has been written, the reference's own lines below do the step -- for the plain
                # Frobenius objective only: beta != 2 and weighted fits have no fall-back, a step the backend cannot take
                # raises)
                if not self._plain_frobenius:
                    raise
                if tap:   # (nothing has been written, the tap included)
                    value = self._energy_function()
        neg, pos = self._backend.reconstruction_gradient_H(self._V, self._W_dict, self._H, s)
        Hs = self._H[s]
        assert neg.shape == Hs.shape and pos.shape == Hs.shape
        if lateral:
            axes = tuple(range(-len(self.atom_shape), 0))
            g = self._backend.convolve_multi_1d(Hs, self._inhibition_kernels_1D, axes)
            if inhibition > 0:
                term = g - Hs               # an activation does not inhibit itself at its own position
                term *= inhibition
                pos += term
            if cross_inhibition > 0:
                term = g.sum(axis=1, keepdims=True) - g   # what all OTHER atoms contribute at this shift
                term *= cross_inhibition / (Hs.shape[1] - 1)
                pos += term
        self._multiplicative_update(Hs, neg, pos, sparsity=sparsity)
        return value

    def _iteration(self, h_args, update_H: bool = True, update_W: bool = True, record: bool = False) -> Optional[float]:
        """One full-batch MU iteration (reference :334-340).  A problem small enough to be launch-latency bound goes to the
        backend as one operation list (one persistent kernel launch per iteration, HIP_Backend.run_schedule).
        record: returns the objective of the (W, H) the iteration starts from -- tapped from the H half step where the
        backend offers that, else (no tap, no H half step, or the one-call path, which keeps its persistent kernel)
        evaluated before the iteration."""
        run = self._scheduler(h_args)
        if run is not None and getattr(self._backend, 'prefers_schedule', lambda *_: False)(self._H):
            value = self._energy_function() if record else None
            ops = ([('H', sliceNone)] if update_H else []) + ([('G', sliceNone, 0., 1.), ('W',)] if update_W else [])
            acc = self._iteration_acc
            if acc is None or acc.shape[1:] != self._W.shape or acc.dtype != self._W.dtype or acc.device != self._W.device:
                self._iteration_acc = self._backend.new_gradient_accumulator(self._W)
            run(self._V, self._W, self._H, ops, self._iteration_acc, sparsity=h_args['sparsity'], eps=self.eps)
            return value
        value = self._update_H(record=record, **h_args) if update_H else (self._energy_function() if record else None)
        if update_W:
            self._update_W()
        if record and value is None:
            # the H half step left every local sample's objective in the buffer: the one place that waits for it
            value = self._backend.read_objective(self._objective_buf)
        return value

    def _initialize_matrices(self, V: np.ndarray, keep_W: bool, weights: Optional[np.ndarray] = None):
        """weights: None, or the materialised weights of _weights_of (the backend receives the keyword only then)."""
        self._V = V
        self._iteration_acc = None    # (sized and typed for the W of ONE fit: a refit may change dtype or device)
        self._objective_buf = None    # (one value per local sample of ONE fit)
        self._weighted = weights is not None
        # (the host copy, kept only for atom_terms / atom_gram / their divergence forms / the triggered sums on a backend
        # without the hooks)
        hooks = [getattr(self._backend, name, None) for name in ('atom_terms', 'atom_gram', 'atom_divergence_terms',
                                                                 'atom_divergence_gram', 'triggered_sums')]
        self._weights = weights if None in hooks else None
        kw = {} if weights is None else {'weights': weights}
        if self._transforms is not None:
            kw['transforms'] = self._transforms
        self._W, self._H = self._backend.initialize(self._V, self.atom_shape, self.n_atoms,
                                                    self._W if keep_W else None, self._axes_W_normalization, **kw)
        self._W_eff = None if self._transforms is None else self._backend.expand_W(self._W, self._transforms)

    def _init_fit(self, V: np.ndarray, keep_W: bool, G: Optional[np.ndarray]) -> None:
        # (the existing call form when unweighted: callers that wrap _initialize_matrices keep working)
        if G is None:
            self._initialize_matrices(V, keep_W)
        else:
            self._initialize_matrices(V, keep_W, weights=G)

    def _report(self, what: str, step: int, progress_callback: Optional[ProgressCallback]) -> bool:
        """Returns False when the callback asks to stop."""
        if progress_callback is not None:
            return bool(progress_callback(self, step))
        if self._logger.isEnabledFor(logging.INFO):
            self._logger.info(f'{what}: {step}\tEnergy function: {self._energy_function()}')
        return True

    def _weights_of(self, V: np.ndarray, weights) -> Optional[np.ndarray]:
        """None, or ``weights`` broadcast to V's shape and materialised in V's dtype -- after the checks: a backend without
        weighted objectives and volumes raise NotImplementedError; weights that do not broadcast, negative, NaN or inf
        (in V's dtype) raise ValueError."""
        if weights is None:
            return None
        if not getattr(self._backend, 'supports_weights', False):
            raise NotImplementedError(f'weights: the backend {type(self._backend).__name__} does not support weighted '
                                      f'objectives')
        if len(self.atom_shape) == 3:
            raise NotImplementedError('weights: weighted objectives cover 1 or 2 shift axes, not volumes')
        try:
            G = np.broadcast_to(np.asarray(weights), V.shape)
        except ValueError as exc:
            raise ValueError(f'weights of shape {np.shape(weights)} do not broadcast to V.shape {V.shape}') from exc
        if G.dtype.kind not in 'biuf':
            raise ValueError(f'weights must be real numbers, not {G.dtype}')
        with np.errstate(over='ignore', invalid='ignore'):
            G = G.astype(V.dtype)   # (a copy: the backend owns it)
        if not np.all(np.isfinite(G)):
            raise ValueError(f'weights must be finite (in {V.dtype.name})')
        if np.any(G < 0):
            raise ValueError('weights must be non-negative')
        return G

    @staticmethod
    def _check_samples(V: np.ndarray, G: Optional[np.ndarray]):
        # (entries of zero weight are not data: any value, NaN included, is accepted there)
        assert np.all(V >= 0) if G is None else np.all((V >= 0) | (G == 0))

    def _check_beta_samples(self, V: np.ndarray, G: Optional[np.ndarray] = None):
        # (R^(beta-1) and V / R of a zero sample: the divergence is not defined there -- scikit-learn refuses the same)
        if self._beta <= 0 and np.any(V == 0 if G is None else (V == 0) & (G > 0)):
            raise ValueError(f'beta_loss={self._beta} <= 0 needs V without zeros')

    def _begin_fit(self, V: np.ndarray, weights, keep_W: bool, objective_every, tol, sparsity_H: float,
                   inhibition_strength: float, cross_atom_inhibition_strength: float):
        """What fit_batch and fit_minibatches share before their loops: the arguments checked, W and H initialised, an empty
        history.  Returns (objective_every, tol, h_args)."""
        every, tol = self._convergence_args(objective_every, tol)
        G = self._weights_of(V, weights)
        self._check_samples(V, G)
        assert sparsity_H >= 0 and inhibition_strength >= 0 and cross_atom_inhibition_strength >= 0
        self._check_beta_samples(V, G)
        self._init_fit(V, keep_W, G)
        self._begin_history()
        return every, tol, dict(sparsity=sparsity_H, inhibition=inhibition_strength,
                                cross_inhibition=cross_atom_inhibition_strength)

    # -- full batch (reference :282-348) ------------------------------------------------------------------------
    def fit_batch(self, V: np.ndarray, n_iterations: int = 1000, update_H: bool = True, update_W: bool = True,
                  keep_W: bool = False, sparsity_H: float = 0., inhibition_strength: float = 0.,
                  cross_atom_inhibition_strength: float = 0., progress_callback: ProgressCallback = None,
                  weights=None, objective_every: Optional[int] = None, tol: Optional[float] = None):
        assert update_H or update_W
        every, tol, h_args = self._begin_fit(V, weights, keep_W, objective_every, tol, sparsity_H, inhibition_strength,
                                             cross_atom_inhibition_strength)
        n_done = 0
        for iteration in range(n_iterations):
            record = every is not None and iteration % every == 0
            value = self._iteration(h_args, update_H, update_W, record=record)
            n_done = iteration + 1
            stop = record and self._record(iteration, value, tol)
            if not self._report('Iteration', iteration, progress_callback) or stop:
                break
        self._end_history(n_done)
        self._logger.info('TNMF finished.')

    # -- mini batches (reference :350-504) ----------------------------------------------------------------------
    def fit_minibatches(self, V: np.ndarray, algorithm: MiniBatchAlgorithm = MiniBatchAlgorithm.ASG_MU,
                        batch_size: int = 3, n_epochs: int = 1000, sag_lambda: float = 0.2, keep_W: bool = False,
                        sparsity_H: float = 0., inhibition_strength: float = 0.,
                        cross_atom_inhibition_strength: float = 0., progress_callback: ProgressCallback = None,
                        weights=None, objective_every: Optional[int] = None, tol: Optional[float] = None):
        assert isinstance(algorithm, MiniBatchAlgorithm)
        # The reference decides whether to shuffle V with `algorithm in (5, 6, 7, 8)` (:410), an Enum-vs-int test
        # that is never true, so V is never shuffled; this front end keeps that behaviour.
        every, tol, h_args = self._begin_fit(V, weights, keep_W, objective_every, tol, sparsity_H, inhibition_strength,
                                             cross_atom_inhibition_strength)
        plan = getattr(self._backend, 'minibatch_slices', None)
        batches = plan(batch_size) if plan is not None else _sequential_minibatches(len(self._V), batch_size)
        epoch_fn = {
            MiniBatchAlgorithm.Cyclic_MU: self._epoch_cyclic,
            MiniBatchAlgorithm.ASG_MU: self._epoch_asg,
            MiniBatchAlgorithm.GSG_MU: self._epoch_gsg,
            MiniBatchAlgorithm.ASAG_MU: self._epoch_asag,
            MiniBatchAlgorithm.GSAG_MU: self._epoch_gsag,
        }[algorithm]
        state = None
        n_done = 0
        for epoch in range(n_epochs):
            # (the exact objective at the epoch boundary: one reconstruction per recorded epoch; the epochs run as they do)
            stop = every is not None and epoch % every == 0 and self._record(epoch, self._energy_function(), tol)
            state = epoch_fn(state, batches, h_args, sag_lambda)
            n_done = epoch + 1
            if not self._report('Epoch', epoch, progress_callback) or stop:
                break
        self._end_history(n_done)
        self._logger.info('MiniBatch TNMF finished.')

    def _local_gradient_W(self):
        """The backend's hook for this rank's [neg | pos] of the W gradient (not yet summed over ranks), or None.  With
        transforms: the gradient of the effective atoms folded onto W (M-atom buffers from here on: the accumulators and
        the collective never see the effective ones)."""
        if self._transforms is not None:
            return lambda V, W, H, s: self._backend.fold_gradient_W(
                self._backend.local_gradient_W(V, self._W_eff, H, s, **self._objective()), self._transforms)
        if not self._plain_frobenius:
            return lambda V, W, H, s: self._backend.local_gradient_W(V, W, H, s, **self._objective())
        return self._fused('local_gradient_W')

    def _blend_gradient_W(self, acc, a: float, b: float, s: slice):
        """acc <- a * acc + b * grad_W(batch s), the gradient summed over the ranks (reference :444-455); a == 0: acc is still
        the reference's integer 0 and the result a new accumulator."""
        if not self._plain_frobenius:
            negpos = self._backend.all_reduce_gradient_W(self._local_gradient_W()(self._V, self._W, self._H, s))
            neg, pos = negpos[0], negpos[1]
        else:
            neg, pos = self._backend.reconstruction_gradient_W(self._V, self._W, self._H, s)
        if a == 0:
            # `0 + g` / `0 * (1 - lam) + lam * g`
            return [neg, pos] if b == 1 else [b * neg, b * pos]
        if a == 1 and b == 1:
            acc[0] += neg
            acc[1] += pos
        else:
            acc[0] *= a
            acc[1] *= a
            acc[0] += b * neg
            acc[1] += b * pos
        return acc

    def _apply_accumulated_W(self, acc):
        # NB: like the reference (:232), the update adds eps to the `pos` accumulator in place
        self._multiplicative_update(self._W, acc[0], acc[1], normalization_axes=self._axes_W_normalization)
        self._expand_W()

    # An epoch of a mini-batch schedule is stated ONCE, as a list of operations -- ('H', batch), ('G', batch, a, b) for
    # acc = a * acc + b * gradient_W(batch), ('W',) for the W update from acc: the epoch functions below only build that list,
    # _run_ops executes it.  Where the backend offers that and no lateral term is on (those go through tnmf_hip_update_H_ex
    # batch by batch) the list is ONE call of the backend (HIP_Backend.run_schedule -> tnmf_hip_run_schedule).
    def _scheduler(self, h_args):
        run = self._fused('run_schedule') if self._use_schedules and self._plain_frobenius else None
        if run is None or not getattr(self._backend, 'supports_schedules', False):
            return None
        if h_args['inhibition'] > 0 or h_args['cross_inhibition'] > 0:
            return None
        return run

    @staticmethod
    def _blend_coefficients(first: bool, lam: float):
        """(a, b) of acc = a * acc + b * g for reference :444-455; `first`: acc is still the integer 0 of :482/:495."""
        if first:
            return 0., (1. if lam == 1 else lam)
        return (1., 1.) if lam == 1 else (1. - lam, lam)

    def _summing_hook(self, ops, h_args):
        """_local_gradient_W() when the list only sums gradients for the W update that ends it -- this rank's [neg | pos]
        can then be summed as they are and cross the collective ONCE per list -- else False."""
        local = None if h_args['inhibition'] > 0 or h_args['cross_inhibition'] > 0 else self._local_gradient_W()
        if local is None or ops[-1][0] != 'W':
            return False
        sums = all(op[0] == 'H' or (op[0] == 'G' and op[2] in (0, 1) and op[3] == 1) for op in ops[:-1])
        return local if sums else False

    def _run_ops(self, ops, h_args, state=None, carried=False):
        """Execute the operation list of one epoch.  `carried`: the accumulator outlives the list (ASAG / GSAG) -- `state` is
        the one the previous epoch returned, None before the first; returns the accumulator, None when not carried.

        One call of the backend where _scheduler offers it.  Otherwise step by step with the half steps above:
        * a run of H steps is issued per contiguous run of samples (_joined: they commute), a single one as it is (an empty
          tail batch of a multi-rank plan included);
        * ('G', s, 0, 1) directly followed by ('W',), accumulator not carried, is the W half step _update_W(s);
        * a list that only sums gradients, not carried, takes the local sums of _summing_hook: one all-reduce at 'W';
        * anything else blends the reduced gradient of every batch into the accumulator (_blend_gradient_W)."""
        run = self._scheduler(h_args)
        if run is not None and len(ops) > 1:   # (not a Cyclic epoch without batches, a lone ('W',))
            acc = self._backend.new_gradient_accumulator(self._W) if state is None else state
            run(self._V, self._W, self._H, ops, acc, sparsity=h_args['sparsity'], eps=self.eps)
            return acc if carried else None
        acc, blend = state, None
        local = False if carried else None   # (None: decided by the first gradient that is no W half step of its own)
        rest = iter(ops + [(None,)])         # (a sentinel: every operation has a next one to look at)
        op = next(rest)
        while op[0] is not None:
            kind, nxt = op[0], next(rest)
            if kind == 'H':
                if nxt[0] == 'H':
                    span = [op[1], nxt[1]]
                    for nxt in rest:
                        if nxt[0] != 'H':
                            break
                        span.append(nxt[1])
                    for s in _joined(span):
                        self._update_H(s, **h_args)
                else:
                    self._update_H(op[1], **h_args)
            elif kind == 'G':
                _, s, a, b = op
                if a == 0 and b == 1 and nxt[0] == 'W' and not carried:
                    self._update_W(s)
                    nxt = next(rest)
                else:
                    if local is None:
                        local, blend = self._summing_hook(ops, h_args), self._fused('blend_gradient_W')
                    if not local:
                        acc = self._blend_gradient_W(acc, a, b, s)
                    else:
                        part = local(self._V, self._W, self._H, s)
                        if a == 0:
                            acc = part
                        elif blend is not None:
                            blend(acc, part, 1., 1.)
                        else:
                            acc += part
            elif local:
                self._backend.apply_W(self._W, self._backend.all_reduce_gradient_W(acc), eps=self.eps)
                self._expand_W()
            else:
                self._apply_accumulated_W(acc)
            op = nxt
        return acc if carried else None

    def _epoch_cyclic(self, _state, batches, h_args, _lam):
        """Algorithm 4: H per batch, W once per epoch from the summed gradient (reference :457-465)."""
        ops = []
        for i, batch in enumerate(batches):
            ops += [('H', batch), ('G', batch, 0. if i == 0 else 1., 1.)]
        return self._run_ops(ops + [('W',)], h_args)

    def _epoch_asg(self, _state, batches, h_args, _lam):
        """Algorithm 5: H and W after every (shuffled) batch (reference :467-472)."""
        ops = []
        for batch in _permuted(batches):
            ops += [('H', batch), ('G', batch, 0., 1.), ('W',)]
        return self._run_ops(ops, h_args)

    def _epoch_gsg(self, _state, batches, h_args, _lam):
        """Algorithm 6: H for every shuffled batch, W from the last batch only (reference :474-479)."""
        order = _permuted(batches)
        ops = [('H', b) for b in order] + [('G', order[-1] if len(order) else slice(0, 0), 0., 1.), ('W',)]
        return self._run_ops(ops, h_args)

    def _epoch_asag(self, state, batches, h_args, lam):
        """Algorithm 7: running average of the W gradient over batches AND epochs (reference :481-491)."""
        first = state is None
        ops = []
        for batch in _permuted(batches):
            ops += [('H', batch), ('G', batch) + self._blend_coefficients(first, lam), ('W',)]
            first = False
        return self._run_ops(ops, h_args, state, carried=True)

    def _epoch_gsag(self, state, batches, h_args, lam):
        """Algorithm 8: H for every batch, averaged gradient refreshed from the last one (reference :493-504)."""
        order = _permuted(batches)
        ops = [('H', b) for b in order]
        ops += [('G', order[-1] if len(order) else slice(0, 0)) + self._blend_coefficients(state is None, lam), ('W',)]
        return self._run_ops(ops, h_args, state, carried=True)

    # -- streaming (reference :506-523) ---------------------------------------------------------------------------
    def fit_stream(self, V: Iterator[np.ndarray], subsample_size: int = 3, max_subsamples: int = None, **kwargs):
        if kwargs.get('weights') is not None:
            raise ValueError('fit_stream takes no weights (an iterator of samples has no matching weights)')
        for isub in itertools.count(0):
            subsample = list(itertools.islice(V, subsample_size))
            if not subsample:
                self._logger.info('Sample iterator exhausted. TNMF on full iterator finished.')
                return
            self._logger.info(f'Processing subsample {isub}.')
            self.fit(np.asarray(subsample), keep_W=True, **kwargs)   # only W carries over
            if max_subsamples is not None and isub == max_subsamples - 1:
                self._logger.info(f'Processed {max_subsamples} subsamples. TNMF on iterator will stop.')
                return

    def fit(self, V: Union[np.ndarray, Iterable[np.ndarray]], **kwargs):
        """Dispatch on the keyword arguments exactly like the reference (:525-531)."""
        if 'subsample_size' in kwargs or 'max_subsamples' in kwargs:
            self.fit_stream(iter(V), **kwargs)
        elif 'batch_size' in kwargs or 'algorithm' in kwargs:
            self.fit_minibatches(V, **kwargs)
        else:
            self.fit_batch(V, **kwargs)
