"""
The backend interface of the factorisation front-end -- the drop-in boundary of this package.

It mirrors, name for name and argument for argument, the abstract class the reference's front-end programs
against (reference: tnmf/backends/_Backend.py:13-130), so that a backend written for one works under the other:

==============================  =====================================  ===========================================
method                          reference                              contract
==============================  =====================================  ===========================================
initialize                      _Backend.py:35-44                      -> (W, H) backend-native, H drawn before W
reconstruct                     _Backend.py:120-122                    R[n,c,*D]
reconstruction_gradient_H       _Backend.py:110-118                    (neg, pos), each of H[s]'s shape
reconstruction_gradient_W       _Backend.py:100-108                    (neg, pos), each of W's shape
partial_reconstruct             _Backend.py:124-125                    one atom's contribution to R
reconstruction_energy           _Backend.py:127-130                    1/2 sum (V - R)^2 as a Python float
normalize                       _Backend.py:75-77                      in place over `axis`
convolve_multi_1d               _Backend.py:79-81                      separable zero-padded convolution
to_ndarray                      _Backend.py:46-49                      backend-native -> numpy.ndarray
==============================  =====================================  ===========================================

Optional hooks a backend may add (the front-end uses them when present):
``multiplicative_update``, ``fused_update_H``, ``fused_update_W``.  A backend that declares ``supports_weights`` takes
``initialize(..., weights=G)`` and then evaluates the weighted objective in its hooks and energy.  A backend that
declares ``supports_transforms`` takes ``initialize(..., transforms=name)`` (tnmf_amd/transforms.py): H then has
``n_atoms * T`` effective atoms while W keeps ``n_atoms``, and it offers ``expand_W(W, name, W_eff=None) -> W_eff``,
``fold_gradient_W(negpos_eff, name) -> negpos`` and ``fused_update_W_transformed(V, W, W_eff, H, s, name, eps, beta)``;
every other hook is called with W_eff in the place of W.  A backend that declares ``supports_atom_operators`` as well
takes an ``AtomOperators`` (tnmf_amd/transforms.py) wherever those hooks take a group name.  A backend that declares
``supports_objective_tap`` reads the objective off the reconstruction its H half step computes anyway: it offers
``new_objective_buffer() -> buf`` (one float64 per local sample, backend-native), takes ``fused_update_H(...,
objective_out=buf)`` -- passed only on the iterations that record; the step's slice selects the part written, with each
sample's objective at the (W, H) passed in -- and ``read_objective(buf) -> float``, the only call that waits: the sum in
sample order, over all ranks.  ``sample_objective(V, W, H, beta, eps)`` -> one float64 per local sample, host side.
``atom_terms(V, W, H, group) -> (a, b)`` (float64 ``[n_local, n_planes / group]``, host): what each block of ``group``
planes of W -- an atom in all its orientations -- explains of the local samples under the Frobenius objective, with the
weights when they are bound (include/tnmf_hip.h, "atom terms"); without it ``atom_terms`` / ``atom_gains`` run
``atom_terms_numpy`` (tnmf_amd/atoms_host.py) on the host.
``atom_gram(V, W, H, group) -> (a, B)`` (float64 ``[n_local, Mo]`` and ``[n_local, Mo, Mo]``, ``Mo = n_planes / group``,
host): ``a`` as above and ``B[n, m, m'] = sum G R_m R_m'``, symmetric, in the order of H's atoms (include/tnmf_hip.h, "atom
Gram"); without it ``atom_gram`` and what builds on it (``atom_overlaps``, ``atom_set_gain``, ``atom_scales``,
``rescale_atoms``, ``atom_elimination``) run ``atom_gram_numpy`` (tnmf_amd/atoms_host.py) on the host.
``atom_divergence_terms(V, W, H, group, beta, eps) -> (a, b, gain)`` and ``atom_divergence_gram(V, W, H, group, beta, eps)
-> (a, B)``: the same shapes under the beta-divergence (include/tnmf_hip.h, "atom terms, beta"); without them the front
end's ``atom_divergence_*`` run ``atom_divergence_terms_numpy`` / ``atom_divergence_gram_numpy`` on the host.
A backend that declares ``supports_sources`` offers ``source_parts(V, W, H, plane_order, source_start, output) -> out``
(backend-native ``[n_local, S, C, *D]``: source g is the planes ``plane_order[source_start[g]:source_start[g + 1]]``, the
planes in no source count in the total only; ``output`` one of 'contribution', 'mask', 'masked', with the ``eps`` keyword)
and ``dominant_parts(V, W, H, plane_order, source_start) -> (label, share)`` (include/tnmf_hip.h, "sources"); either may
raise ``NotImplementedError``, and then, as without the hooks, ``separate`` / ``dominant_source`` run ``separate_numpy`` /
``dominant_numpy`` (tnmf_amd/sources_host.py) on the host.
A backend that declares ``supports_peaks`` offers ``find_peaks(H, threshold, radius, group) -> (idx, val)``: the ascending
flat C-order indices (int64, host) in H's shape [n, P, *S] and the values of the detections of its native H
(include/tnmf_hip.h, "detections"); without it ``detections()`` searches ``to_ndarray(H)`` on the host.
``activation_correlogram(H, max_lag, per_sample=False) -> C`` (float64 ``[P, P, *(2 L + 1)]`` or ``[n, P, P, *(2 L + 1)]``,
host): the correlogram of its native H (include/tnmf_hip.h, "activation correlogram"); it may raise ``NotImplementedError``,
and then, as without the hook, ``activation_correlogram()`` runs ``activation_correlogram_numpy``
(tnmf_amd/correlogram_host.py) on the host.
A backend with ``supports_triggered = True`` offers ``triggered_field(V, W, H, source) -> Y`` (its native array ``[n, C, *D]``:
the field 'data', 'reconstruction' or 'residual', times the bound weights when there are any, or 'weights') and
``triggered_sums(H, Y, margin, power=1, per_sample=False) -> X`` (float64 ``[P, F, *(A + 2 m)]`` or ``[n, P, F, *(A + 2 m)]``,
host): the triggered sums of its native H and that field (include/tnmf_hip.h, "triggered sums"); ``triggered_sums`` may
raise ``NotImplementedError``, and then, as without the flag, the front end runs ``triggered_sums_numpy``
(tnmf_amd/triggered_host.py) on the host.
A backend that declares ``supports_events`` works on lists of events (local sample, plane of the effective dictionary,
shift in its H, strength; include/tnmf_hip.h, "events"): ``render_events(W, sample, plane, shift, strength) -> R``
(backend-native ``[n_local, C, *D]``) and ``refit_events(V, W, sample, plane, shift, strength, n_iterations, sparsity=0.,
eps=1e-9) -> strength`` (backend-native ``[K]``); without them ``reconstruct_detections`` / ``refit_detections`` run
``events_numpy`` on the host.  It may also offer ``event_gains(V, W, sample, plane, shift, strength) -> ndarray[K]`` (float64,
host): what each event explains; without it ``detection_gains`` runs ``events_gain_numpy`` on the host.  And
``event_landscape(V, W, sample, plane, shift, strength) -> (a, b)`` (float64 ``[K, 3^k]``, host): every event at its
neighbouring shifts (include/tnmf_hip.h, "landscape"); without it ``detection_landscape`` runs ``events_landscape_numpy``.
And ``event_alternatives(V, W, sample, plane, shift, strength, n_alt, stride) -> (a, b)`` (float64 ``[K, n_alt]``, host): every
event under the other planes of its block at its own shift (include/tnmf_hip.h, "alternatives"); without it
``detection_alternatives`` runs ``events_alternatives_numpy``.
And ``solve_events(V, W, sample, plane, shift, strength, tol, max_iterations, check_every=10) -> (strength, info)``
(backend-native float64 ``[K]``; info: iterations, kkt, converged, nnz, history ``[checks, 2]``): the strengths that minimise
the Frobenius objective on the fixed support (include/tnmf_hip.h, "events: exact strengths"); without it ``solve_detections``
runs ``events_gram_numpy`` and ``events_solve_numpy``.  A ``pursue_events`` hook takes ``solve=(tol, max_iterations)`` when
the front end asks for ``strengths='solve'``.
And ``event_errors(V, W, sample, plane, shift, strength, max_component) -> (d, b, residual_energy, info)`` (backend-native
float64 ``[K]`` twice, a float; info: n_active, n_components, largest_component, n_singular, rounds, row_size ``[K]``): the
diagonal of the inverse of the active block of the Gram matrix, the diagonal of the matrix and ``||V - R(list)||^2``
(include/tnmf_hip.h, "events: standard errors"); without it ``detection_errors`` runs ``events_gram_numpy`` and
``events_inverse_diag_numpy``.
"""
import abc
from typing import Optional, Sequence, Tuple, Union

import numpy as np

sliceNone = slice(None)

Axes = Optional[Union[int, Tuple[int, ...]]]


def shift_shape(reconstruction_mode: str, sample_shape: Sequence[int], atom_shape: Sequence[int]) -> Tuple[int, ...]:
    """Shape of the activation (shift) axes of H for a reconstruction mode (reference: _Backend.py:60-73)."""
    pairs = list(zip(sample_shape, atom_shape))
    if reconstruction_mode == 'valid':
        return tuple(int(d + a - 1) for d, a in pairs)
    if reconstruction_mode == 'full':
        return tuple(int(d - a + 1) for d, a in pairs)
    if reconstruction_mode in ('same', 'circular', 'reflect'):
        return tuple(int(d) for d, _ in pairs)
    raise ValueError(f'unknown reconstruction mode {reconstruction_mode!r}')


def axis_images(mode: str, u, a: int, s: int):
    """(first, second, has_second): the positions in the padded frame ``[D + A - 1]`` that copy the shifts ``u`` of one axis
    (atom extent ``a``, shift extent ``s``) -- the table of include/tnmf_hip.h, "events".  ``has_second`` says where the
    second one exists: a 'circular' shift in the wrap zone, a 'reflect' shift in the mirror zone; None for the modes that
    have none.  Elementwise ``+ - >= <= &`` only: numpy arrays and torch tensors alike."""
    if mode == 'circular':
        return u + (a - 1), u - (s - (a - 1)), u >= s - (a - 1)
    if mode == 'reflect':
        return u + (a - 1), (a - 1) - u, (u >= 1) & (u <= a - 1)
    return (u if mode == 'valid' else u + (a - 1)), None, None


class Backend(abc.ABC):
    """Numerical back end of :class:`tnmf_amd.TransformInvariantNMF.TransformInvariantNMF`."""

    # takes an AtomOperators as ``transforms`` (with ``supports_transforms``): arbitrary non-negative linear atom maps
    supports_atom_operators = False
    # fused_update_H takes ``objective_out`` (with new_objective_buffer / read_objective): the objective tap
    supports_objective_tap = False
    # offers ``find_peaks``: the detections are found where H lives
    supports_peaks = False
    # offers ``render_events`` / ``refit_events``: detections are rendered and refitted without a dense H
    supports_events = False

    def __init__(self, reconstruction_mode: str = 'valid'):
        self._reconstruction_mode = reconstruction_mode
        self.atom_shape = None
        self.n_samples = None
        self.n_channels = None
        self._sample_shape = None
        self._transform_shape = None
        self._n_shift_dimensions = None

    # -- set-up -------------------------------------------------------------------------------------------
    def initialize(self, V: np.ndarray, atom_shape: Tuple[int, ...], n_atoms: int, W=None,
                   axes_W_normalization: Axes = None, weights: Optional[np.ndarray] = None,
                   transforms: Optional[str] = None):
        """``weights``: elementwise weights of V's shape and dtype for the weighted objective, only for a backend that
        declares ``supports_weights`` (handed on to ``_initialize_matrices`` as the keyword ``weights``).  ``transforms``:
        a transform group, only for a backend that declares ``supports_transforms``, or an ``AtomOperators``, only for one
        that declares ``supports_atom_operators`` as well (handed on as the keyword ``transforms``)."""
        self._set_dimensions(V, atom_shape)
        kw = {}
        if weights is not None:
            if not getattr(self, 'supports_weights', False):
                raise NotImplementedError(f'the backend {type(self).__name__} does not support weighted objectives')
            kw['weights'] = weights
        if transforms is not None:
            if not getattr(self, 'supports_transforms', False):
                raise NotImplementedError(f'the backend {type(self).__name__} does not support transform groups')
            if not isinstance(transforms, str) and not getattr(self, 'supports_atom_operators', False):
                raise NotImplementedError(f'the backend {type(self).__name__} does not support atom operators')
            kw['transforms'] = transforms
        return self._initialize_matrices(V, atom_shape, n_atoms, W, axes_W_normalization, **kw)

    def _set_dimensions(self, V: np.ndarray, atom_shape: Tuple[int, ...]) -> None:
        self.atom_shape = tuple(atom_shape)
        self.n_samples, self.n_channels = V.shape[0], V.shape[1]
        self._sample_shape = tuple(V.shape[2:])
        self._transform_shape = shift_shape(self._reconstruction_mode, self._sample_shape, self.atom_shape)
        self._n_shift_dimensions = len(self.atom_shape)

    @abc.abstractmethod
    def _initialize_matrices(self, V, atom_shape, n_atoms, W, axes_W_normalization):
        ...

    # -- the three primitives -----------------------------------------------------------------------------
    @abc.abstractmethod
    def reconstruct(self, W, H):
        ...

    @abc.abstractmethod
    def reconstruction_gradient_H(self, V, W, H, s: slice = sliceNone):
        ...

    @abc.abstractmethod
    def reconstruction_gradient_W(self, V, W, H, s: slice = sliceNone):
        ...

    # -- derived / auxiliary ------------------------------------------------------------------------------
    def partial_reconstruct(self, W, H, i_atom: int):
        return self.reconstruct(W[i_atom:i_atom + 1], H[:, i_atom:i_atom + 1])

    @abc.abstractmethod
    def reconstruction_energy(self, V, W, H) -> float:
        ...

    @abc.abstractmethod
    def normalize(self, arr, axis: Axes = None) -> None:
        ...

    def convolve_multi_1d(self, arr, kernels, axes):
        raise NotImplementedError

    @staticmethod
    @abc.abstractmethod
    def to_ndarray(arr) -> np.ndarray:
        ...
