"""
The 'hip' backend: every primitive of the shift-invariant MU loop runs as a hand-written gfx950 kernel of
libtnmf_hip.so (C ABI: include/tnmf_hip.h), called through ctypes on raw device pointers.

PyTorch is plumbing here: it owns the device buffers (``torch.Tensor``), the current HIP stream and -- for the
sample-sharded multi-GPU mode -- the RCCL all-reduce (``torch.distributed``).  No arithmetic of the hot path is
done by torch, and there is no CPU fallback: without the built library or without a GPU the constructor raises.

Reference counterparts: tnmf/backends/NumPy.py (the 'valid'-mode direct-convolution backend whose results this
backend reproduces) and tnmf/backends/_Backend.py (the interface).
"""
from typing import Optional, Sequence, Tuple

import ctypes
import itertools
import weakref

import numpy as np
import torch

from .. import _lib, sharding, transforms as _transforms
from ..events_host import pursuit_loop
from ..patches_host import fold_table
from ._Backend import Backend, axis_images, sliceNone

_DTYPES = {np.dtype('float32'): (torch.float32, 0), np.dtype('float64'): (torch.float64, 1)}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _EventSpan:
    """Brackets a launch with two HIP events on the current stream when the backend's timeline is on."""

    def __init__(self, backend, name):
        self.backend, self.name = backend, name

    def __enter__(self):
        if self.backend._timeline is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream(self.backend._device))
        return self

    def __exit__(self, *exc):
        if self.backend._timeline is not None:
            self.e1.record(torch.cuda.current_stream(self.backend._device))
            self.backend._timeline.append((self.name, self.e0, self.e1))
            self.backend._timeline_paths[self.name] = self.backend.last_path
        return False


class HIP_Backend(Backend):
    r"""
    MI355X backend for 'valid'-mode shift-invariant NMF (1-D and 2-D shifts, float32 and float64).

    Parameters
    ----------
    reconstruction_mode : ``'valid'`` (the fused matrix-core path), or ``'full'`` / ``'circular'`` / ``'reflect'``: these
           pad the activations (tnmf_hip_pad_H), run the same 'valid' kernels on the padded tensor and fold the H gradient
           back (tnmf_hip_fold_H) -- the padding table of the reference's _PyTorchBackend.py:42-52
    device : CUDA/HIP device index or ``torch.device``; default: the current device
    path : ``'auto'`` | ``'generic'`` | ``'mfma'`` | ``'split'`` | ``'fft'`` | ``'hybrid'`` -- kernel family
           (``'auto'`` = the fastest dispatch that keeps W and H within 1e-5 of the float64 reference; ``'mfma'`` = direct
           kernels on the exact f32-input MFMA; ``'split'`` = direct kernels with the H update on the bf16 matrix
           cores through exact 3 x bf16 operand splits; ``'fft'`` = frequency-domain formulation, the algorithm of the
           reference's default backend -- **W-only in float32**: W and the energy stay within 1e-5 of the float64
           reference, the activations do NOT (float32 transform noise in the quotient of two small gradients; measured
           up to 2e-3 of max|H| after 5 iterations); in float64 everything is within 1e-10; ``'hybrid'`` = FFT family
           for reconstruct and the W gradient, direct H update)
    split : ``True`` (default) lets ``'auto'`` / ``'hybrid'`` run the H update on the bf16 matrix cores (3 x bf16 splits,
           float32-grade); ``False`` keeps it on the exact f32-input MFMA
    init : ``'reference'`` draws H then W from the global legacy NumPy RNG exactly like the reference
           (_Backend.py:92-95); ``'device'`` draws them with the device generator (fast, not seed-compatible)
    process_group : a ``torch.distributed`` group, ``True`` for the default group, ``None``, or any object with
           ``rank``, ``world_size`` and ``all_reduce_sum(tensor)`` (a collective injected by the caller; the tests use
           an in-process one to run two ranks on one GPU).  With a group the sample axis is sharded in contiguous blocks
           over the ranks: this rank keeps V[n0:n1] and H[n0:n1], the W-gradient numerator/denominator is all-reduced
           (sum) before it is returned, the energy likewise.
    reduce : ``'all_reduce'`` (one RCCL all-reduce; the order of the additions is RCCL's choice of protocol) or
           ``'ordered'``: all-gather of the ranks' [neg | pos] buffers, then their sum in rank order by a library kernel --
           bit-identical on every rank and from run to run.  The buffers are 37-393 KB: either way the
           exchange is latency-bound.
    persistent : how tnmf_hip_run_schedule may run a TINY resident problem (BASELINE config 1): ``1`` (default) one
           persistent kernel per call whose grid is sized by an occupancy query -- its grid-wide barriers need every
           workgroup resident, which the library checks instead of assuming; ``2`` the same through
           hipLaunchCooperativeKernel; ``0`` never (walk the list operation by operation: say so when the GPU is shared
           with other processes).  Where the persistent grid does not fit the library falls back by itself.
    sharded_input : ``False`` (default): every rank passes the GLOBAL ``V`` to ``fit`` / ``initialize`` and keeps its
           block (sharding.shard_bounds).  ``True``: every rank passes ONLY ITS OWN samples (the global array never
           exists on any host: 3.2 GB x 8 at BASELINE config 5); the ranks' blocks follow each other in rank order and may
           differ in length (one all-reduce of the per-rank counts at initialize).
    """

    def __init__(self, reconstruction_mode: str = 'valid', device=None, path: str = 'auto', init: str = 'reference',
                 process_group=None, split: bool = True, reduce: str = 'all_reduce', sharded_input: bool = False,
                 persistent: int = 1):
        if reconstruction_mode not in _lib.MODES:
            raise ValueError(f'Unsupported reconstruction mode "{reconstruction_mode}". '
                             f'Please choose "valid", "full", "circular", or "reflect".')
        super().__init__(reconstruction_mode=reconstruction_mode)
        self._mode = _lib.MODES[reconstruction_mode]
        self._lib = _lib.load()  # raises when the extension is not built
        if not torch.cuda.is_available():
            raise RuntimeError('The hip backend needs a GPU (torch.cuda.is_available() is False); there is no CPU path.')
        if init not in ('reference', 'device'):
            raise ValueError(f'init must be "reference" or "device", not {init!r}')
        self._device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if self._device.index is None:
            self._device = torch.device('cuda', torch.cuda.current_device())
        if reduce not in ('all_reduce', 'ordered'):
            raise ValueError(f'reduce must be "all_reduce" or "ordered", not {reduce!r}')
        self._init_mode = init
        self._reduce = reduce
        self._sharded_input = bool(sharded_input)
        self._counts = None         # samples per rank (sharded_input: as handed in; else sharding.shard_bounds)
        self._counts_pending = None
        self._ctx = ctypes.c_void_p()
        self._ops_handles = {}      # AtomOperators.key -> (operators, library handle on self._ctx)
        self._fold_tables = {}      # group name or AtomOperators.key -> the device table of tnmf_hip_events_patches
        _lib.check(self._lib.tnmf_hip_ctx_create(self._device.index, ctypes.byref(self._ctx)), 'tnmf_hip_ctx_create')
        _lib.check(self._lib.tnmf_hip_ctx_set_path(self._ctx, _lib.PATHS[path]), 'tnmf_hip_ctx_set_path')
        _lib.check(self._lib.tnmf_hip_ctx_set_split(self._ctx, 1 if split else 0), 'tnmf_hip_ctx_set_split')
        _lib.check(self._lib.tnmf_hip_ctx_set_persistent(self._ctx, int(persistent)), 'tnmf_hip_ctx_set_persistent')
        # FFT family: the library may reuse the row spectra of H between the fused half steps (it updated H itself);
        # every other entry point below declares H as possibly changed first (_foreign_H).
        _lib.check(self._lib.tnmf_hip_ctx_set_cache(self._ctx, 1 if reconstruction_mode == 'valid' else 0),
                   'tnmf_hip_ctx_set_cache')

        self._group = None
        self._collective = None     # injected: object with rank / world_size / all_reduce_sum(tensor)
        self._rank, self._world = 0, 1
        if process_group is not None and process_group is not False:
            if hasattr(process_group, 'all_reduce_sum'):
                self._collective = process_group
                self._rank, self._world = int(process_group.rank), int(process_group.world_size)
            else:
                import torch.distributed as dist
                self._group = dist.group.WORLD if process_group is True else process_group
                self._rank, self._world = dist.get_rank(self._group), dist.get_world_size(self._group)

        self._torch_dtype = None
        self._dtype_code = None
        self._V_dev = None          # this rank's samples, device resident
        self._G_dev = None          # this rank's weights (weighted fit), laid out like _V_dev; None: unweighted
        self._shard = (0, 0)        # [n0, n1) of the global sample axis held by this rank
        self._R_scratch = None
        self._negpos = None
        self._timeline = None
        self._timeline_paths = {}
        self._cached_H = None       # (weakref of the base tensor, data_ptr, shape, torch version counter)

    def __del__(self):
        try:
            for _, handle in getattr(self, '_ops_handles', {}).values():
                self._lib.tnmf_hip_atom_ops_destroy(handle)
            self._ops_handles = {}
            if getattr(self, '_ctx', None) is not None and self._ctx.value:
                self._lib.tnmf_hip_ctx_destroy(self._ctx)
                self._ctx = ctypes.c_void_p()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    # -- helpers --------------------------------------------------------------------------------------------
    @property
    def device(self) -> torch.device:
        return self._device

    @property
    def shard(self) -> Tuple[int, int]:
        """Global sample range [n0, n1) resident on this rank."""
        return self._shard

    @property
    def last_path(self) -> str:
        return self._lib.tnmf_hip_ctx_last_path(self._ctx).decode()

    @property
    def last_schedule_persistent(self) -> bool:
        """Whether the last run_schedule call ran as ONE persistent kernel launch (else: operation by operation)."""
        return bool(self._lib.tnmf_hip_ctx_last_schedule_persistent(self._ctx))

    @property
    def cache_counters(self) -> dict:
        """Row-transform passes of the FFT family over H / V that ran, and that the spectrum cache made unnecessary."""
        out = (ctypes.c_ulonglong * 4)()
        _lib.check(self._lib.tnmf_hip_ctx_cache_counters(self._ctx, ctypes.byref(out)), 'tnmf_hip_ctx_cache_counters')
        return dict(h_runs=int(out[0]), h_hits=int(out[1]), v_runs=int(out[2]), v_hits=int(out[3]))

    def _foreign_H(self) -> None:
        """H of the coming call may have been written by someone else: drop cached spectra (FFT family)."""
        self._lib.tnmf_hip_ctx_invalidate(self._ctx)
        self._cached_H = None

    # The FFT family keeps the row spectra of the activations it transformed or updated (tnmf_hip_ctx_set_cache), per
    # sample of the resident H it was told about (tnmf_hip_ctx_bind in initialize(): mini-batch slices H[s] share one
    # cache, the way the reference's caching backend keeps one cache per slice, NumPy_CachingFFT.py:143-158).  The library
    # can only key that cache on raw pointers; validity is therefore owned HERE: after each fused call the identity of
    # the storage (weak reference to the base tensor of the slice) and torch's version counter are recorded; a fused call
    # on other storage, or on the same storage written by any torch operation in between (which bumps the counter; the
    # library's own writes through the raw pointer do not) -- whichever samples that write hit -- invalidates first.
    @staticmethod
    def _h_key(Hs: torch.Tensor):
        base = Hs._base if Hs._base is not None else Hs
        return base, (base.data_ptr(), tuple(base.shape), base._version)

    def _validate_H_cache(self, Hs: torch.Tensor, W: Optional[torch.Tensor] = None) -> None:
        """Before a fused call: drop what the library cached about H (and about the dictionary W, whose spectra it keeps
        between W updates) unless both are the tensors, unwritten by torch, that the last fused call left behind."""
        c = self._cached_H
        if c is None:
            self._lib.tnmf_hip_ctx_invalidate(self._ctx)
            return
        base, key = self._h_key(Hs)
        w_same = W is None or (c[2] is not None and c[2]() is W and c[3] == (W.data_ptr(), W._version))
        if c[0]() is not base or c[1] != key or not w_same:
            self._lib.tnmf_hip_ctx_invalidate(self._ctx)
            self._cached_H = None

    def _note_H_cache(self, Hs: torch.Tensor, W: Optional[torch.Tensor] = None) -> None:
        base, key = self._h_key(Hs)
        self._cached_H = (weakref.ref(base), key, None if W is None else weakref.ref(W),
                          None if W is None else (W.data_ptr(), W._version))

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)

    # -- optional per-kernel timeline (bench.py): HIP events on the stream the kernels are launched on ----------
    def start_timeline(self) -> None:
        """From now on the fused half steps launch their reconstruct separately and bracket every kernel group with
        HIP events (recorded on the launch stream, no host synchronisation)."""
        self._timeline = []
        self._timeline_paths = {}

    @property
    def timeline_paths(self):
        """{kernel group: kernel family it ran on} of the last timeline."""
        return dict(self._timeline_paths)

    def stop_timeline(self):
        """-> {name: [milliseconds per launch, ...]}; synchronises."""
        torch.cuda.synchronize(self._device)
        out = {}
        for name, e0, e1 in self._timeline or []:
            out.setdefault(name, []).append(e0.elapsed_time(e1))
        self._timeline = None
        return out

    def _timed(self, name: str):
        return _EventSpan(self, name)

    def _geom(self, n: int, n_atoms: int, h_row_stride: int = 0):
        return _lib.make_geom(n, n_atoms, self.n_channels, self._sample_shape, self.atom_shape, self._dtype_code,
                              h_row_stride)

    def _check_W(self, W: torch.Tensor):
        assert W.is_cuda and W.is_contiguous() and W.dtype == self._torch_dtype
        assert tuple(W.shape[1:]) == (self.n_channels,) + self.atom_shape

    def _check_H(self, H: torch.Tensor, n_atoms: int):
        assert H.is_cuda and H.dtype == self._torch_dtype
        assert tuple(H.shape[1:]) == (n_atoms,) + self._transform_shape

    # Activations may live in storage whose rows are padded to whole cache lines (initialize() asks the library:
    # tnmf_hip_ctx_h_row_stride); the tensor the front end holds is then a VIEW of that storage -- every torch operation
    # of the reference's front end works on it unchanged -- and the C ABI is told the row stride (tnmf_hip_geom).
    @staticmethod
    def _row_stride(H: torch.Tensor) -> Optional[int]:
        """Row stride (elements) of a C-contiguous or row-padded [N, M, *shift] tensor; None for any other layout."""
        if H.is_contiguous():
            return 0
        if H.dim() != 4 or H.stride(3) != 1:
            return None
        ld = H.stride(2)
        n, m, hy, hx = H.shape
        ok = ld >= hx and (m <= 1 or H.stride(1) == hy * ld) and (n <= 1 or H.stride(0) == m * hy * ld)
        if hy <= 1:   # (no row stride to read off a single row)
            return None
        return ld if ok else None

    def _call_H(self, Hs: torch.Tensor, inplace: bool, call) -> bool:
        """call(H tensor, row stride) -> return code of a library function that reads (inplace: updates) Hs.  A
        row-padded Hs goes in as it is; when the kernel family of the call wants C-contiguous activations
        (TNMF_E_STRIDE: nothing has been touched) or the layout is something else, a contiguous copy goes in instead and,
        for an in-place call, is copied back.  Returns whether a copy was used (the library then saw a temporary: the
        caller drops what it cached about it)."""
        ld = self._row_stride(Hs)
        if ld is not None:
            rc, where = call(Hs, ld)
            if not (rc == _lib.E_STRIDE and ld != 0):
                _lib.check(rc, where)
                return False
        Hc = Hs.contiguous()
        rc, where = call(Hc, 0)
        _lib.check(rc, where)
        if inplace:
            Hs.copy_(Hc)
        return True

    def _call_resident_H(self, Hs: torch.Tensor, W: torch.Tensor, inplace: bool, call, lateral: bool = False) -> None:
        """_call_H on a slice of the resident activations, with the spectrum-cache bookkeeping around it: before the call
        the cache is validated ('valid' mode) or dropped; after it the library's spectra are noted as those of (Hs, W),
        or dropped when they belong to a temporary copy or to another reconstruction mode.  A library error drops them
        too; TNMF_E_UNSUPPORTED with lateral terms becomes NotImplementedError (the library answers it before it writes H:
        inhibition kernels too long for the lateral-term kernel's LDS tile, or planes beyond its 32-bit offsets)."""
        if self._mode == 0:
            self._validate_H_cache(Hs, W)   # (the library drops the spectra of the samples it updates itself)
        else:
            self._foreign_H()
        try:
            copied = self._call_H(Hs, inplace, call)
        except _lib.TnmfHipError as exc:
            self._foreign_H()
            if exc.code == _lib.E_UNSUPPORTED and lateral:
                raise NotImplementedError('lateral terms outside the fused kernel') from exc
            raise
        if copied or self._mode != 0:
            self._foreign_H()   # (the spectra the library may have kept belong to a temporary, or are not cached)
        elif Hs.shape[0]:
            self._note_H_cache(Hs, W)

    # beta-divergence objectives (the hooks' `beta`): the multiplicative updates of D_beta are those of the Frobenius
    # objective with (V, R) replaced by the fields Q = V * R~^(beta-2), P = R~^(beta-1) of R~ = R + eps
    # (include/tnmf_hip.h, "beta-divergence objectives"); beta == 2 is the Frobenius call itself.  Volumes are not covered.
    supports_beta_loss = True

    def _check_beta(self, beta: float) -> None:
        if beta != 2. and len(self.atom_shape) == 3:
            raise NotImplementedError('beta-divergence objectives other than the Frobenius norm: 1 or 2 shift axes only')

    # weighted objectives (initialize(..., weights=G)): sum G * D_beta(V | R), the fields above multiplied by G
    # (include/tnmf_hip.h, "weighted objectives").  While weights are bound every half step and the energy use G[s] of the
    # resident weights, at any beta; the unweighted gradient primitive of H refuses.  Volumes are not covered.
    supports_weights = True

    # transform groups (initialize(..., transforms=name)): the resident activations have n_atoms * T effective atoms, W
    # keeps n_atoms; the front end holds W_eff = expand_W(W) and hands it to every hook in the place of W.  The W step is
    # fused_update_W_transformed: gradient of W_eff, folded onto W before the collective, MU + normalise, expanded again
    # (include/tnmf_hip.h, "transform groups").  Volumes are not covered.
    supports_transforms = True

    # atom operators (initialize(..., transforms=AtomOperators)): the same hooks with arbitrary non-negative linear maps of
    # the atoms (include/tnmf_hip.h, "atom operators").  One library handle per operator set and context, made at first
    # use, reused across steps and fits, freed with the context.
    supports_atom_operators = True

    def _group_id(self, transforms: str) -> int:
        if len(self.atom_shape) == 3:
            raise NotImplementedError('transforms: 1 or 2 shift axes only')
        return _lib.GROUPS[_transforms.check(transforms, self.atom_shape)]

    def _ops_handle(self, ops) -> ctypes.c_void_p:
        """The library handle of the operators ``ops`` on this context (made at first use)."""
        if len(self.atom_shape) == 3:
            raise NotImplementedError('transforms: 1 or 2 shift axes only')
        _transforms.check(ops, self.atom_shape)
        entry = self._ops_handles.get(ops.key)
        if entry is None:
            t, out_px, in_px, w = ops.entries
            ci = ctypes.c_int
            arr = [np.ascontiguousarray(a, dtype=np.int32) for a in (t, out_px, in_px)]
            wd = np.ascontiguousarray(w, dtype=np.float64)
            A = (ci * len(ops.atom_shape))(*ops.atom_shape)
            handle = ctypes.c_void_p()
            _lib.check(self._lib.tnmf_hip_atom_ops_create(
                self._ctx, len(ops.atom_shape), A, ops.T, ops.nnz,
                *[a.ctypes.data_as(ctypes.POINTER(ci)) for a in arr],
                wd.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(handle)), 'tnmf_hip_atom_ops_create')
            entry = self._ops_handles[ops.key] = (ops, handle)
        return entry[1]

    def _fold_table(self, transforms):
        """(fold_ptr, fold_src, fold_w, T): the table of tnmf_hip_events_patches for ``transforms`` on this device (None:
        no table, T = 1), built once per (transforms, atom shape) (patches_host.fold_table) and kept beside the operator
        handles.  The atom shape is part of the key: the table of a group name has T * prod(A) + 1 row starts, the kernel
        reads it by the geometry of the call, and a backend may be initialised again with atoms of another shape."""
        if transforms is None:
            return None, None, None, 1
        if len(self.atom_shape) == 3:
            raise NotImplementedError('transforms: 1 or 2 shift axes only')
        transforms = _transforms.check(transforms, self.atom_shape)
        key = (transforms.key if isinstance(transforms, _transforms.AtomOperators) else transforms, tuple(self.atom_shape))
        entry = self._fold_tables.get(key)
        if entry is None:
            ptr, src, w, T = fold_table(transforms, self.atom_shape)
            entry = self._fold_tables[key] = tuple(torch.from_numpy(a).to(self._device) for a in (ptr, src, w)) + (T,)
        return entry

    def _transform_arg(self, transforms):
        """-> (entry point family, its argument): ('group', TNMF_GROUP_*) for a group name, ('ops', handle) for an
        AtomOperators."""
        if isinstance(transforms, _transforms.AtomOperators):
            return 'ops', self._ops_handle(transforms)
        return 'group', self._group_id(transforms)

    def _G(self, ls: slice):
        return None if self._G_dev is None else _ptr(self._G_dev[ls])

    def _local(self, s: slice) -> slice:
        """Slices address this rank's resident samples (all samples when there is no process group)."""
        lo, hi, step = s.indices(self._shard[1] - self._shard[0])
        assert step == 1, 'sample slices must be contiguous'
        return slice(lo, max(lo, hi))

    @property
    def n_local_samples(self) -> int:
        return self._shard[1] - self._shard[0]

    def minibatch_slices(self, batch_size: Optional[int]):
        """
        Sequential mini-batches in this rank's sample coordinates.  With a process group, global batch j is the
        union of every rank's local batch j: each rank contributes ceil(batch_size / world) of its own samples,
        and all ranks get the same number of batches (possibly empty at the tail) so their all-reduces pair up.
        Without a group this is the reference's sequential split (TransformInvariantNMF.py:29-37).
        """
        return sharding.local_minibatches(self.n_samples, self._rank, self._world, batch_size, counts=self._counts)

    @property
    def _padded_shape(self) -> Tuple[int, ...]:
        return tuple(d + a - 1 for d, a in zip(self._sample_shape, self.atom_shape))

    def _pad(self, H: torch.Tensor) -> torch.Tensor:
        """Activations of this mode -> the padded tensor every kernel works on (identity for 'valid')."""
        if self._mode == 0:
            return H
        if not H.is_contiguous():
            H = H.contiguous()
        assert tuple(H.shape[2:]) == self._transform_shape
        Hp = torch.empty(tuple(H.shape[:2]) + self._padded_shape, dtype=H.dtype, device=H.device)
        g = self._geom(H.shape[0], H.shape[1])
        _lib.check(self._lib.tnmf_hip_pad_H(self._ctx, ctypes.byref(g), self._mode, _ptr(H), _ptr(Hp), self._stream()),
                   'tnmf_hip_pad_H')
        return Hp

    def _fold(self, Gp: torch.Tensor) -> torch.Tensor:
        """Gradient w.r.t. the padded activations -> gradient w.r.t. the activations (adjoint of _pad)."""
        if self._mode == 0:
            return Gp
        G = torch.empty(tuple(Gp.shape[:2]) + self._transform_shape, dtype=Gp.dtype, device=Gp.device)
        g = self._geom(Gp.shape[0], Gp.shape[1])
        _lib.check(self._lib.tnmf_hip_fold_H(self._ctx, ctypes.byref(g), self._mode, _ptr(Gp), _ptr(G), self._stream()),
                   'tnmf_hip_fold_H')
        return G

    def _all_reduce(self, t: torch.Tensor) -> None:
        if self._world > 1 and self._reduce == 'ordered':
            # fixed-order reduction: gather every rank's buffer, then add them up in rank order on the device
            # (tnmf_hip_sum_parts) -- the same bits on every rank and from run to run, whatever RCCL protocol an all-reduce
            # of this size would have used
            parts = (self._collective.all_gather(t) if self._collective is not None
                     else sharding.all_gather(t, self._group))
            assert t.is_contiguous() and parts.is_contiguous() and parts.shape[0] == self._world
            code = _DTYPES[np.dtype(str(t.dtype).replace('torch.', ''))][1]
            _lib.check(self._lib.tnmf_hip_sum_parts(self._ctx, code, _ptr(parts), self._world, t.numel(), _ptr(t),
                                                    self._stream()), 'tnmf_hip_sum_parts')
            return
        if self._collective is not None:
            self._collective.all_reduce_sum(t)
        else:
            sharding.all_reduce_sum(t, self._group)

    # -- set-up ---------------------------------------------------------------------------------------------
    def exchange_sample_counts(self, n_local: int):
        """sharded_input: the ranks' sample counts in rank order (one small all-reduce).  initialize() does this itself;
        a caller that has to serialise the seeded draw of several ranks inside one process (the tests) does it first --
        the result is kept for the next initialize() with that many samples."""
        counts = torch.zeros(self._world, dtype=torch.float64, device=self._device)
        counts[self._rank] = n_local
        saved, self._reduce = self._reduce, 'all_reduce'
        try:
            self._all_reduce(counts)
        finally:
            self._reduce = saved
        self._counts_pending = [int(round(c)) for c in counts.tolist()]
        return self._counts_pending

    def _initialize_matrices(self, V: np.ndarray, atom_shape, n_atoms: int, W=None, axes_W_normalization=None,
                             weights: Optional[np.ndarray] = None, transforms=None):
        """With ``transforms`` (a group name or an AtomOperators): H (and everything sized by it) has n_atoms * T
        effective atoms, W has n_atoms; H is drawn first, then W, as without."""
        if transforms is not None:
            self._transform_arg(transforms)
        n_dict = n_atoms
        n_atoms = n_atoms * (1 if transforms is None else _transforms.size(transforms))
        if V.dtype not in _DTYPES:
            raise TypeError(f'the hip backend computes in float32 or float64, V has dtype {V.dtype}')
        if len(atom_shape) not in (1, 2, 3):   # (3: volumes, on the direct kernels of tnmf_amd/csrc/volume.hip)
            raise NotImplementedError('the hip backend supports 1, 2 or 3 shift dimensions')
        if weights is not None:
            if len(atom_shape) == 3:
                raise NotImplementedError('weighted objectives: 1 or 2 shift axes only')
            if weights.shape != V.shape or weights.dtype != V.dtype:
                raise ValueError(f'weights must have the shape {V.shape} and dtype {V.dtype} of V (the front end '
                                 f'broadcasts them)')
        self._G_dev = None
        self._torch_dtype, self._dtype_code = _DTYPES[V.dtype]
        self._foreign_H()
        if self._sharded_input and self._world > 1:
            # V is this rank's block already: the ranks tell each other their sample counts (one small all-reduce)
            pending, self._counts_pending = self._counts_pending, None
            if pending is None or pending[self._rank] != V.shape[0]:
                pending = self.exchange_sample_counts(V.shape[0])
                self._counts_pending = None
            self._counts = pending
            self.n_samples = N = sum(self._counts)
            n0 = sum(self._counts[:self._rank])
            n0, n1 = self._shard = (n0, n0 + self._counts[self._rank])
            V_local, G_local = V, weights
        else:
            N = self.n_samples
            n0, n1 = self._shard = sharding.shard_bounds(N, self._rank, self._world)
            self._counts = None
            V_local, G_local = V[n0:n1], None if weights is None else weights[n0:n1]
        with torch.cuda.device(self._device):
            self._V_dev = torch.as_tensor(np.ascontiguousarray(V_local)).to(self._device)
            if G_local is not None:
                self._G_dev = torch.as_tensor(np.ascontiguousarray(G_local)).to(self._device)
                self._V_dev.masked_fill_(self._G_dev == 0, 0)   # (never data: whatever V held there is not kept)
            ld = ctypes.c_int(0)
            if self._mode == 0 and len(atom_shape) == 2 and n1 > n0:
                _lib.check(self._lib.tnmf_hip_ctx_h_row_stride(self._ctx, ctypes.byref(self._geom(n1 - n0, n_atoms)),
                                                               ctypes.byref(ld)), 'tnmf_hip_ctx_h_row_stride')
            if ld.value > self._transform_shape[-1]:
                # rows padded to whole 128-byte lines (zeros; never read as data): H is a view of the padded storage
                store = torch.zeros((n1 - n0, n_atoms, self._transform_shape[0], ld.value), dtype=self._torch_dtype,
                                    device=self._device)
                H = store[..., :self._transform_shape[-1]]
            else:
                H = torch.empty((n1 - n0, n_atoms) + self._transform_shape, dtype=self._torch_dtype,
                                device=self._device)
            if self._init_mode == 'device':
                H.uniform_(0, 1).neg_().add_(1)
            else:
                for i, h in sharding.reference_init_stream(N, (n_atoms,) + self._transform_shape, self._shard, V.dtype):
                    H[i].copy_(torch.from_numpy(h))
            if W is None:
                if self._init_mode == 'device' and self._world == 1:
                    W = torch.empty((n_dict, self.n_channels) + self.atom_shape, dtype=self._torch_dtype,
                                    device=self._device).uniform_(0, 1).neg_().add_(1)
                    self.normalize(W, axes_W_normalization)
                else:
                    W = torch.from_numpy(sharding.reference_init_W(n_dict, self.n_channels, self.atom_shape,
                                                                   V.dtype)).to(self._device)
            else:
                self._check_W(W)
                assert W.shape[0] == n_dict
            self._R_scratch = torch.empty_like(self._V_dev)
            self._negpos = torch.empty((2, n_atoms, self.n_channels) + self.atom_shape, dtype=self._torch_dtype,
                                       device=self._device)
            # the resident problem of this fit: slices H[s] / V[s] of it share the library's spectrum cache
            bound = self._mode == 0 and n1 > n0
            _lib.check(self._lib.tnmf_hip_ctx_bind(
                self._ctx, ctypes.byref(self._geom(n1 - n0, n_atoms, max(ld.value, 0))) if bound else None,
                _ptr(H) if bound else None, _ptr(self._V_dev) if bound else None), 'tnmf_hip_ctx_bind')
            _lib.check(self._lib.tnmf_hip_ctx_reserve(self._ctx, ctypes.byref(self._geom(n1 - n0, n_atoms))),
                       'tnmf_hip_ctx_reserve')
        return W, H

    # -- primitives -----------------------------------------------------------------------------------------
    def reconstruct(self, W: torch.Tensor, H: torch.Tensor) -> torch.Tensor:
        """R = H (*) W, 'valid' part (reference: NumPy.py:122-132) -> tnmf_hip_reconstruct."""
        self._check_W(W)
        self._foreign_H()
        self._check_H(H, W.shape[0])
        H = self._pad(H)
        R = torch.empty((H.shape[0], self.n_channels) + self._sample_shape, dtype=self._torch_dtype, device=self._device)
        self._call_H(H, False, lambda Hc, ld: (self._lib.tnmf_hip_reconstruct(
            self._ctx, ctypes.byref(self._geom(Hc.shape[0], W.shape[0], ld)), _ptr(W), _ptr(Hc), _ptr(R),
            self._stream()), 'tnmf_hip_reconstruct'))
        return R

    def reconstruction_gradient_H(self, V, W: torch.Tensor, H: torch.Tensor, s: slice = sliceNone):
        """(neg, pos) of H[s]'s shape (reference: NumPy.py:93-120) -> tnmf_hip_grad_H.  `V` is the array given to
        initialize(); the device-resident copy is used (precedent: NumPy_CachingFFT.py:259,273).  The gradient of the
        unweighted objective: refused while weights are bound (fused_update_H takes the weighted step)."""
        if self._G_dev is not None:
            raise NotImplementedError('reconstruction_gradient_H is unweighted; a weighted fit steps H through '
                                      'fused_update_H')
        self._check_W(W)
        self._foreign_H()
        ls = self._local(s)
        Hs, Vs = H[ls], self._V_dev[ls]
        self._check_H(Hs, W.shape[0])
        Hs = self._pad(Hs)
        neg = torch.empty(Hs.shape, dtype=Hs.dtype, device=Hs.device)   # (C-contiguous whatever the layout of H)
        pos = torch.empty(Hs.shape, dtype=Hs.dtype, device=Hs.device)
        self._call_H(Hs, False, lambda Hc, ld: (self._lib.tnmf_hip_grad_H(
            self._ctx, ctypes.byref(self._geom(Hc.shape[0], W.shape[0], ld)), _ptr(Vs), None, _ptr(W), _ptr(Hc),
            _ptr(neg), _ptr(pos), self._stream()), 'tnmf_hip_grad_H'))
        return self._fold(neg), self._fold(pos)

    def reconstruction_gradient_W(self, V, W: torch.Tensor, H: torch.Tensor, s: slice = sliceNone):
        """(neg, pos) of W's shape (reference: NumPy.py:69-91) -> tnmf_hip_grad_W_fused; summed over the ranks of
        the process group (one all-reduce of the contiguous [neg | pos] buffer)."""
        self._foreign_H()
        negpos = self.local_gradient_W(V, W, H, s)
        self._all_reduce(negpos)
        return negpos[0], negpos[1]

    def reconstruction_energy(self, V, W: torch.Tensor, H: torch.Tensor, beta: float = 2., eps: float = 1e-9) -> float:
        """1/2 sum (V - R)^2 (reference: _Backend.py:127-130), or for beta != 2 sum D_beta(V | R + eps)
        -> tnmf_hip_energy_beta (+ all-reduce); with weights bound the weighted sum -> tnmf_hip_energy_weighted."""
        self._check_beta(beta)
        self._check_W(W)
        self._foreign_H()
        self._check_H(H, W.shape[0])
        H = self._pad(H)
        out = ctypes.c_double(0.0)
        if self._G_dev is None:
            self._call_H(H, False, lambda Hc, ld: (self._lib.tnmf_hip_energy_beta(
                self._ctx, ctypes.byref(self._geom(Hc.shape[0], W.shape[0], ld)), float(beta), float(eps),
                _ptr(self._V_dev), _ptr(W), _ptr(Hc), ctypes.byref(out), self._stream()), 'tnmf_hip_energy_beta'))
        else:
            self._call_H(H, False, lambda Hc, ld: (self._lib.tnmf_hip_energy_weighted(
                self._ctx, ctypes.byref(self._geom(Hc.shape[0], W.shape[0], ld)), float(beta), float(eps),
                _ptr(self._V_dev), _ptr(self._G_dev), _ptr(W), _ptr(Hc), ctypes.byref(out), self._stream()),
                'tnmf_hip_energy_weighted'))
        if self._world > 1:
            t = torch.tensor([out.value], dtype=torch.float64, device=self._device)
            self._all_reduce(t)
            return float(t.item())
        return float(out.value)

    def partial_reconstruct(self, W, H, i_atom: int):
        return self.reconstruct(W[i_atom:i_atom + 1].contiguous(), H[:, i_atom:i_atom + 1].contiguous())

    def normalize(self, arr: torch.Tensor, axis=None) -> None:
        """arr /= arr.sum(axis, keepdims=True) for W over its atom axes (reference: _Backend.py:75-77)."""
        k = len(self.atom_shape)
        ax = tuple(sorted(a % arr.ndim for a in ((axis,) if isinstance(axis, int) else tuple(axis or ()))))
        if ax != tuple(range(arr.ndim - k, arr.ndim)) or tuple(arr.shape[-k:]) != self.atom_shape:
            raise NotImplementedError('the hip backend normalises dictionaries over their atom axes only')
        assert arr.is_cuda and arr.is_contiguous()
        rows = int(np.prod(arr.shape[:-k]))
        g = _lib.make_geom(0, rows, 1, self._sample_shape, self.atom_shape, self._dtype_code)
        _lib.check(self._lib.tnmf_hip_normalize_W(self._ctx, ctypes.byref(g), _ptr(arr), self._stream()),
                   'tnmf_hip_normalize_W')

    def convolve_multi_1d(self, arr: torch.Tensor, kernels: Sequence[np.ndarray], axes: Sequence[int]) -> torch.Tensor:
        """Separable zero-padded convolution along the shift axes (reference: _NumPyBackend.py:56-64)."""
        k = len(self.atom_shape)
        axes = tuple(a % arr.ndim for a in axes)
        if axes != tuple(range(arr.ndim - k, arr.ndim)) or len(kernels) != k:
            raise NotImplementedError('the hip backend convolves along the shift axes only')
        assert arr.is_cuda
        if not arr.is_contiguous():   # (e.g. row-padded activations)
            arr = arr.contiguous()
        out = torch.empty_like(arr)
        tmp = torch.empty_like(arr) if k >= 2 else None
        ks = [np.ascontiguousarray(kk, dtype=np.float64) for kk in kernels]
        kp = [kk.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for kk in ks]
        if k == 3:
            # volumes: one axis per call, first shift axis first (_NumPyBackend.py:60-62), ping-ponging two buffers so
            # that the third pass lands in `out`
            shp = [int(x) for x in arr.shape]
            src, bufs = arr, [out, tmp, out]
            for i in range(3):
                rows, inner = int(np.prod(shp[:2 + i])), int(np.prod(shp[3 + i:]))
                _lib.check(self._lib.tnmf_hip_convolve_axis(
                    self._ctx, self._dtype_code, rows, shp[2 + i], inner, _ptr(src), _ptr(bufs[i]), kp[i], len(ks[i]),
                    self._stream()), 'tnmf_hip_convolve_axis')
                src = bufs[i]
            return out
        shape = (ctypes.c_int * 2)(*[int(x) for x in arr.shape[-k:]] + [1] * (2 - k))
        rows = int(np.prod(arr.shape[:-k]))
        _lib.check(self._lib.tnmf_hip_convolve_multi_1d(
            self._ctx, self._dtype_code, k, rows, shape, _ptr(arr), _ptr(out), _ptr(tmp), kp[0], len(ks[0]),
            kp[1] if k == 2 else None, len(ks[1]) if k == 2 else 0, self._stream()), 'tnmf_hip_convolve_multi_1d')
        return out

    @staticmethod
    def to_ndarray(arr: torch.Tensor) -> np.ndarray:
        """Device tensor -> host ndarray (with a process group: this rank's shard of H / R)."""
        return np.ascontiguousarray(arr.detach().cpu().numpy())

    # -- optional hooks used by the front-end ---------------------------------------------------------------
    def multiplicative_update(self, arr: torch.Tensor, neg: torch.Tensor, pos: torch.Tensor, regularization: float):
        """pos += reg (in place); arr = arr * neg / pos  (reference: TransformInvariantNMF.py:232-235)."""
        assert neg.is_contiguous() and pos.is_contiguous()
        assert arr.shape == neg.shape == pos.shape
        flat = arr if arr.is_contiguous() else arr.contiguous()   # (a flat elementwise kernel: row-padded H goes through a copy)
        _lib.check(self._lib.tnmf_hip_mu_update(self._ctx, self._dtype_code, _ptr(flat), _ptr(neg), _ptr(pos),
                                                float(regularization), flat.numel(), self._stream()),
                   'tnmf_hip_mu_update')
        if flat is not arr:
            arr.copy_(flat)

    def fused_update_H(self, V, W: torch.Tensor, H: torch.Tensor, s: slice = sliceNone, sparsity: float = 0.,
                       eps: float = 1e-9, inhibition: float = 0., cross_inhibition: float = 0.,
                       inhibition_kernels: Optional[Sequence[np.ndarray]] = None, beta: float = 2.,
                       objective_out: Optional[torch.Tensor] = None) -> None:
        """One H half step, in place (reference: TransformInvariantNMF.py:246-271): 'valid' mode without lateral terms on
        the fused kernels (tnmf_hip_update_H); with lateral inhibition / cross-atom inhibition and for the other
        reconstruction modes through tnmf_hip_update_H_ex, for beta != 2 through tnmf_hip_update_H_beta, with weights
        bound through tnmf_hip_update_H_weighted -- the separable convolution, the lateral terms, the pad, the fold, the
        (weighted) beta-divergence fields and the update all run as kernels of the library.
        objective_out (new_objective_buffer()): objective_out[s] receives each sample's objective at the (W, H) passed in,
        read off the reconstruction the step computes anyway (tnmf_hip_ctx_set_objective_tap); no synchronisation."""
        self._check_beta(beta)
        ls = self._local(s)
        Hs, Vs = H[ls], self._V_dev[ls]
        if objective_out is not None:
            assert objective_out.is_cuda and objective_out.dtype == torch.float64 and objective_out.is_contiguous()
            assert tuple(objective_out.shape) == (self.n_local_samples,)
        if Hs.shape[0] == 0:
            return
        self._check_W(W)
        self._check_H(Hs, W.shape[0])
        Rs = self._R_scratch[ls]
        lateral = inhibition > 0 or cross_inhibition > 0
        Gs = self._G(ls)
        if self._mode == 0 and not lateral and beta == 2. and Gs is None:
            def run(Hc, ld):
                g = self._geom(Hc.shape[0], W.shape[0], ld)
                r_valid = 0
                if self._timeline is not None:
                    with self._timed('reconstruct'):
                        rc = self._lib.tnmf_hip_reconstruct(self._ctx, ctypes.byref(g), _ptr(W), _ptr(Hc), _ptr(Rs),
                                                            self._stream())
                    if rc != 0:
                        return rc, 'tnmf_hip_reconstruct'
                    r_valid = 1
                with self._timed('update_H'):
                    rc = self._lib.tnmf_hip_update_H(self._ctx, ctypes.byref(g), _ptr(Vs), _ptr(W), _ptr(Hc), _ptr(Rs),
                                                     r_valid, float(eps), float(sparsity), self._stream())
                return rc, 'tnmf_hip_update_H'
        else:
            k = len(self.atom_shape)
            ks = [np.ascontiguousarray(kk, dtype=np.float64) for kk in (inhibition_kernels or ())]
            if lateral and len(ks) != k:
                raise ValueError('one inhibition kernel per shift axis')
            kp = [kk.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for kk in ks] + [None, None, None]
            kl = [len(kk) for kk in ks] + [0, 0, 0]

            def run(Hc, ld):
                args = (self._ctx, ctypes.byref(self._geom(Hc.shape[0], W.shape[0], ld)), self._mode, _ptr(Vs), _ptr(W),
                        _ptr(Hc), _ptr(Rs), float(eps), float(sparsity), float(inhibition), float(cross_inhibition),
                        kp[0], kl[0], kp[1], kl[1], kp[2], kl[2])
                with self._timed('update_H'):
                    if Gs is not None:
                        return self._lib.tnmf_hip_update_H_weighted(*args[:4], Gs, *args[4:], float(beta),
                                                                    self._stream()), 'tnmf_hip_update_H_weighted'
                    if beta == 2.:
                        return self._lib.tnmf_hip_update_H_ex(*args, self._stream()), 'tnmf_hip_update_H_ex'
                    return self._lib.tnmf_hip_update_H_beta(*args, float(beta), self._stream()), 'tnmf_hip_update_H_beta'
        if objective_out is None:
            self._call_resident_H(Hs, W, True, run, lateral)
            return
        _lib.check(self._lib.tnmf_hip_ctx_set_objective_tap(self._ctx, _ptr(objective_out[ls])),
                   'tnmf_hip_ctx_set_objective_tap')
        try:
            self._call_resident_H(Hs, W, True, run, lateral)
        finally:
            self._lib.tnmf_hip_ctx_set_objective_tap(self._ctx, None)

    # -- the objective tap ------------------------------------------------------------------------------------------
    # The H half step materialises R = reconstruct(W, H) before anything else: one pass over (V, R[, G]) there gives
    # the objective of the state the iteration starts from, per sample (include/tnmf_hip.h, "per-sample objective and
    # the objective tap").  Writing it is asynchronous; read_objective is the only place that waits.
    supports_objective_tap = True

    def new_objective_buffer(self) -> torch.Tensor:
        """One float64 per local sample on the device, for ``fused_update_H(..., objective_out=)``."""
        return torch.zeros(self.n_local_samples, dtype=torch.float64, device=self._device)

    def read_objective(self, buf: torch.Tensor) -> float:
        """The objective a tapped H half step over all local samples left in ``buf``: one copy of the per-sample values,
        summed in sample order; with several ranks one all-reduce of the scalar (every rank decides alike)."""
        total = 0.0
        for x in buf.cpu().tolist():
            total += x
        if self._world > 1:
            t = torch.tensor([total], dtype=torch.float64, device=self._device)
            self._all_reduce(t)
            return float(t.item())
        return total

    def sample_objective(self, V, W: torch.Tensor, H: torch.Tensor, beta: float = 2., eps: float = 1e-9) -> np.ndarray:
        """[n_local_samples] float64: each local sample's share of reconstruction_energy(V, W, H, beta, eps)
        -> tnmf_hip_sample_objective."""
        self._check_beta(beta)
        self._check_W(W)
        self._foreign_H()
        self._check_H(H, W.shape[0])
        H = self._pad(H)
        out = torch.zeros(H.shape[0], dtype=torch.float64, device=self._device)
        self._call_H(H, False, lambda Hc, ld: (self._lib.tnmf_hip_sample_objective(
            self._ctx, ctypes.byref(self._geom(Hc.shape[0], W.shape[0], ld)), float(beta), float(eps),
            _ptr(self._V_dev), None if self._G_dev is None else _ptr(self._G_dev), _ptr(W), _ptr(Hc), _ptr(out),
            self._stream()), 'tnmf_hip_sample_objective'))
        return out.cpu().numpy()

    def atom_terms(self, V, W: torch.Tensor, H: torch.Tensor, group: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """(a, b), float64 ``[n_local_samples, n_planes / group]`` on the host: what each block of ``group`` planes of W
        (an atom in all its orientations) explains of the resident samples -- ``a = sum G R_m d``, ``b = sum G R_m^2``
        with the bound weights G (include/tnmf_hip.h, "atom terms") -> tnmf_hip_atom_terms: one pass over H, and only the
        two sums per (sample, atom) cross to the host.  The modes other than 'valid' are the 'valid' pass over the padded
        activations."""
        if len(self.atom_shape) == 3:
            raise NotImplementedError('atom gains: 1 or 2 shift axes only')
        self._check_W(W)
        self._foreign_H()
        self._check_H(H, W.shape[0])
        assert H.shape[0] == self.n_local_samples
        H = self._pad(H)
        ab = torch.empty((H.shape[0], W.shape[0] // max(int(group), 1), 2), dtype=torch.float64, device=self._device)
        self._call_H(H, False, lambda Hc, ld: (self._lib.tnmf_hip_atom_terms(
            self._ctx, ctypes.byref(self._geom(Hc.shape[0], W.shape[0], ld)), int(group), _ptr(self._V_dev),
            None if self._G_dev is None else _ptr(self._G_dev), None, _ptr(W), _ptr(Hc), _ptr(ab), self._stream()),
            'tnmf_hip_atom_terms'))
        out = ab.cpu().numpy()
        return np.ascontiguousarray(out[..., 0]), np.ascontiguousarray(out[..., 1])

    def atom_gram(self, V, W: torch.Tensor, H: torch.Tensor, group: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """(a, B), float64 ``[n_local_samples, Mo]`` and ``[n_local_samples, Mo, Mo]`` (``Mo = n_planes / group``) on the
        host: ``a`` of ``atom_terms`` and ``B[n, m, m'] = sum G R_m R_m'`` with the bound weights G (include/tnmf_hip.h,
        "atom Gram") -> tnmf_hip_atom_gram: one pass over H, the contraction over the pixels on the matrix cores, and only
        the sums cross to the host.  The modes other than 'valid' are the 'valid' pass over the padded activations."""
        if len(self.atom_shape) == 3:
            raise NotImplementedError('atom gains: 1 or 2 shift axes only')
        self._check_W(W)
        self._foreign_H()
        self._check_H(H, W.shape[0])
        assert H.shape[0] == self.n_local_samples
        H = self._pad(H)
        Mo = W.shape[0] // max(int(group), 1)
        a = torch.empty((H.shape[0], Mo), dtype=torch.float64, device=self._device)
        B = torch.empty((H.shape[0], Mo, Mo), dtype=torch.float64, device=self._device)
        self._call_H(H, False, lambda Hc, ld: (self._lib.tnmf_hip_atom_gram(
            self._ctx, ctypes.byref(self._geom(Hc.shape[0], W.shape[0], ld)), int(group), _ptr(self._V_dev),
            None if self._G_dev is None else _ptr(self._G_dev), None, _ptr(W), _ptr(Hc), _ptr(a), _ptr(B), self._stream()),
            'tnmf_hip_atom_gram'))
        return a.cpu().numpy(), B.cpu().numpy()

    def atom_divergence_terms(self, V, W: torch.Tensor, H: torch.Tensor, group: int = 1, beta: float = 2.,
                              eps: float = 1e-9) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(a, b, gain), float64 ``[n_local_samples, n_planes / group]`` on the host, under the beta-divergence with the
        bound weights G (include/tnmf_hip.h, "atom terms, beta") -> tnmf_hip_atom_terms_beta: the pass of ``atom_terms``
        with the slope, the curvature and the exact leave-one-out gain of every (sample, atom); ``beta == 2`` gives the
        bits of ``atom_terms`` and ``a + b / 2``."""
        if len(self.atom_shape) == 3:
            raise NotImplementedError('atom gains: 1 or 2 shift axes only')
        self._check_beta(beta)
        self._check_W(W)
        self._foreign_H()
        self._check_H(H, W.shape[0])
        assert H.shape[0] == self.n_local_samples
        H = self._pad(H)
        abg = torch.empty((H.shape[0], W.shape[0] // max(int(group), 1), 3), dtype=torch.float64, device=self._device)
        self._call_H(H, False, lambda Hc, ld: (self._lib.tnmf_hip_atom_terms_beta(
            self._ctx, ctypes.byref(self._geom(Hc.shape[0], W.shape[0], ld)), int(group), float(beta), float(eps),
            _ptr(self._V_dev), None if self._G_dev is None else _ptr(self._G_dev), None, _ptr(W), _ptr(Hc), _ptr(abg),
            self._stream()), 'tnmf_hip_atom_terms_beta'))
        out = abg.cpu().numpy()
        return tuple(np.ascontiguousarray(out[..., k]) for k in range(3))

    def atom_divergence_gram(self, V, W: torch.Tensor, H: torch.Tensor, group: int = 1, beta: float = 2.,
                             eps: float = 1e-9) -> Tuple[np.ndarray, np.ndarray]:
        """(a, B), float64 ``[n_local_samples, Mo]`` and ``[n_local_samples, Mo, Mo]`` on the host: ``a`` of
        ``atom_divergence_terms`` and ``B[n, m, m'] = sum G c R_m R_m'`` under the signed curvature weights of the
        beta-divergence (include/tnmf_hip.h, "atom terms, beta") -> tnmf_hip_atom_gram_beta; ``beta == 2`` gives the bits
        of ``atom_gram``."""
        if len(self.atom_shape) == 3:
            raise NotImplementedError('atom gains: 1 or 2 shift axes only')
        self._check_beta(beta)
        self._check_W(W)
        self._foreign_H()
        self._check_H(H, W.shape[0])
        assert H.shape[0] == self.n_local_samples
        H = self._pad(H)
        Mo = W.shape[0] // max(int(group), 1)
        a = torch.empty((H.shape[0], Mo), dtype=torch.float64, device=self._device)
        B = torch.empty((H.shape[0], Mo, Mo), dtype=torch.float64, device=self._device)
        self._call_H(H, False, lambda Hc, ld: (self._lib.tnmf_hip_atom_gram_beta(
            self._ctx, ctypes.byref(self._geom(Hc.shape[0], W.shape[0], ld)), int(group), float(beta), float(eps),
            _ptr(self._V_dev), None if self._G_dev is None else _ptr(self._G_dev), None, _ptr(W), _ptr(Hc), _ptr(a),
            _ptr(B), self._stream()), 'tnmf_hip_atom_gram_beta'))
        return a.cpu().numpy(), B.cpu().numpy()

    # -- sources ----------------------------------------------------------------------------------------------------------
    # The per-source signals of the resident samples (include/tnmf_hip.h, "sources"): one pass over H on the walk of the
    # atom terms, the planes in the order the sources list them; the result stays on the device until the caller converts it.
    supports_sources = True

    def _atom_sources(self, W: torch.Tensor, H: torch.Tensor, plane_order, source_start, emit: int, eps: float, out, label,
                      share) -> None:
        """tnmf_hip_atom_sources on the padded activations, the two int32 tables built on the device; TNMF_E_UNSUPPORTED
        (answered before anything is written) becomes NotImplementedError."""
        if len(self.atom_shape) == 3:
            raise NotImplementedError('separate: 1 or 2 shift axes only')
        self._check_W(W)
        self._foreign_H()
        self._check_H(H, W.shape[0])
        assert H.shape[0] == self.n_local_samples
        H = self._pad(H)
        order = torch.as_tensor(np.ascontiguousarray(plane_order, dtype=np.int32), device=self._device)
        start = torch.as_tensor(np.ascontiguousarray(source_start, dtype=np.int32), device=self._device)
        try:
            self._call_H(H, False, lambda Hc, ld: (self._lib.tnmf_hip_atom_sources(
                self._ctx, ctypes.byref(self._geom(Hc.shape[0], W.shape[0], ld)), int(start.numel()) - 1, _ptr(order),
                int(order.numel()), _ptr(start), int(emit), float(eps), _ptr(self._V_dev), _ptr(W), _ptr(Hc), _ptr(out),
                _ptr(label), _ptr(share), self._stream()), 'tnmf_hip_atom_sources'))
        except _lib.TnmfHipError as exc:
            if exc.code == _lib.E_UNSUPPORTED:
                raise NotImplementedError('sources: the atom is beyond the fused kernel') from exc
            raise

    def source_parts(self, V, W: torch.Tensor, H: torch.Tensor, plane_order, source_start, output: str = 'masked',
                     eps: float = 1e-9) -> torch.Tensor:
        """``[n_local_samples, S, C, *D]`` on the device: per source g -- the planes
        ``plane_order[source_start[g]:source_start[g + 1]]`` of W and H -- its 'contribution' ``r_g`` to R, its 'mask'
        ``r_g / (total + eps)`` or the 'masked' samples ``V * mask``, ``total`` being the sum over every plane
        -> tnmf_hip_atom_sources.  The modes other than 'valid' are the 'valid' pass over the padded activations."""
        emit = _lib.SOURCE_OUTPUTS[output]
        assert emit != _lib.SOURCE_OUTPUTS['dominant']
        out = torch.empty((self.n_local_samples, len(source_start) - 1, self.n_channels) + tuple(self._sample_shape),
                          dtype=self._torch_dtype, device=self._device)
        self._atom_sources(W, H, plane_order, source_start, emit, eps, out, None, None)
        return out

    def dominant_parts(self, V, W: torch.Tensor, H: torch.Tensor, plane_order, source_start,
                       eps: float = 1e-9) -> Tuple[torch.Tensor, torch.Tensor]:
        """(label int32, share) ``[n_local_samples, *D]`` on the device: per pixel the source with the largest contribution
        summed over the channels (the lowest index of a tie; -1 where the total is 0) and that sum over the total + eps
        -> tnmf_hip_atom_sources."""
        shape = (self.n_local_samples,) + tuple(self._sample_shape)
        label = torch.empty(shape, dtype=torch.int32, device=self._device)
        share = torch.empty(shape, dtype=self._torch_dtype, device=self._device)
        self._atom_sources(W, H, plane_order, source_start, _lib.SOURCE_OUTPUTS['dominant'], eps, None, label, share)
        return label, share

    # -- detections -----------------------------------------------------------------------------------------------------
    # The peaks of H are found and compacted on the device (include/tnmf_hip.h, "detections"): only the list of
    # (index, value) pairs crosses to the host, never H.
    supports_peaks = True

    def find_peaks(self, H: torch.Tensor, threshold: float, radius: Sequence[int], group: int = 1,
                   capacity: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(idx, val): the flat C-order indices in H's shape [n, P, *S], ascending, and the values of the detections of H
        -- the resident activations, a mini-batch view H[s] of them, row-padded or not -> tnmf_hip_find_peaks.  The list is
        sized by a guess (``capacity``; default: 1/256 of H); when the kernel counts more, it runs once more with the
        exact size.  Sorted by index on the device."""
        k = len(self.atom_shape)
        assert H.is_cuda and H.dtype == self._torch_dtype and H.dim() == 2 + k and len(radius) == k
        ld = self._row_stride(H)
        if ld is None:
            H, ld = H.contiguous(), 0
        n, P = int(H.shape[0]), int(H.shape[1])
        # (the shift shape is H's own, whatever the reconstruction mode: D = S, A = 1)
        g = _lib.make_geom(n, P, self.n_channels, tuple(H.shape[2:]), (1,) * k, self._dtype_code, ld)
        rad = (ctypes.c_int * 3)(*[min(int(r), 2 ** 31 - 1) for r in radius])
        count = torch.zeros(1, dtype=torch.int64, device=self._device)
        cap = max(4096, H.numel() // 256) if capacity is None else int(capacity)
        while True:
            idx = torch.empty(cap, dtype=torch.int64, device=self._device)
            val = torch.empty(cap, dtype=self._torch_dtype, device=self._device)
            with self._timed('find_peaks'):
                _lib.check(self._lib.tnmf_hip_find_peaks(self._ctx, ctypes.byref(g), _ptr(H), float(threshold), rad,
                                                         int(group), _ptr(idx), _ptr(val), cap, _ptr(count),
                                                         self._stream()), 'tnmf_hip_find_peaks')
            total = int(count.item())
            if total <= cap:
                break
            cap = total
        idx, order = torch.sort(idx[:total])
        return idx.cpu().numpy(), val[:total][order].cpu().numpy()

    # -- activation correlogram ------------------------------------------------------------------------------------------
    # Which planes of H co-occur, and at what offset (include/tnmf_hip.h, "activation correlogram"): one pass over H on the
    # f64 matrix cores, and only the [P, P, lags] sums cross to the host.
    CORRELOGRAM_MAX_LAG = {1: 1023, 2: 63}   # correlogram.h: kCorrMaxLag1, kCorrMaxLag2

    def activation_correlogram(self, H: torch.Tensor, max_lag: Sequence[int], per_sample: bool = False) -> np.ndarray:
        """``C[p, q, D] = sum_n sum_u H[n, p, u] H[n, q, u + D]`` for ``|D_k| <= max_lag[k]``, float64
        ``[P, P, *(2 L + 1)]`` on the host, or per sample ``[n, P, P, *(2 L + 1)]`` -- of the resident activations as they
        are, row-padded or not, in any reconstruction mode -> tnmf_hip_activation_correlogram.  NotImplementedError for
        volumes and for a lag beyond the library's limit."""
        k = len(self.atom_shape)
        if k == 3:
            raise NotImplementedError('activation correlogram: 1 or 2 shift axes only')
        assert H.is_cuda and H.dtype == self._torch_dtype and H.dim() == 2 + k and len(max_lag) == k
        limit = self.CORRELOGRAM_MAX_LAG[k]
        if any(int(x) > limit for x in max_lag):
            raise NotImplementedError(f'activation correlogram: max_lag {tuple(max_lag)!r} is beyond the limit of {limit} '
                                      f'per axis on {k} shift ax{"is" if k == 1 else "es"}')
        ld = self._row_stride(H)
        if ld is None:
            H, ld = H.contiguous(), 0
        n, P = int(H.shape[0]), int(H.shape[1])
        # (the shift shape is H's own, whatever the reconstruction mode: D = S, A = 1)
        g = _lib.make_geom(n, P, self.n_channels, tuple(H.shape[2:]), (1,) * k, self._dtype_code, ld)
        lags = (ctypes.c_int * 3)(*[int(x) for x in max_lag])
        shape = ((n,) if per_sample else ()) + (P, P) + tuple(2 * int(x) + 1 for x in max_lag)
        C = torch.empty(shape, dtype=torch.float64, device=self._device)
        with self._timed('activation_correlogram'):
            _lib.check(self._lib.tnmf_hip_activation_correlogram(self._ctx, ctypes.byref(g), _ptr(H), lags,
                                                                 int(bool(per_sample)), _ptr(C), self._stream()),
                       'tnmf_hip_activation_correlogram')
        return C.cpu().numpy()

    # -- triggered sums --------------------------------------------------------------------------------------------------
    # The data around the places where a plane fires, on a window larger than the atom (include/tnmf_hip.h, "triggered
    # sums"): one pass over the padded H and a field of the samples' shape on the f64 matrix cores, and only the
    # [P, F, window] sums cross to the host.  The work buffer is this backend's, not the context's.
    supports_triggered = True
    TRIGGERED_MAX_WINDOW = _lib.TRIGGERED_MAX_WINDOW

    def triggered_field(self, V, W: torch.Tensor, H: torch.Tensor, source: str) -> torch.Tensor:
        """The field ``[n, C, *D]`` of ``source``: 'data' (the resident samples), 'reconstruction', 'residual' (their
        difference) -- each times the bound weights when there are any -- or 'weights' (the weights; ones without)."""
        if source == 'weights':
            return torch.ones_like(self._V_dev) if self._G_dev is None else self._G_dev
        if source == 'data':
            Y = self._V_dev
        elif source == 'reconstruction':
            Y = self.reconstruct(W, H)
        elif source == 'residual':
            Y = self._V_dev - self.reconstruct(W, H)
        else:
            raise ValueError(f'unknown source {source!r}')
        return Y if self._G_dev is None else Y * self._G_dev

    def triggered_sums(self, H: torch.Tensor, Y: torch.Tensor, margin: Sequence[int], power: int = 1,
                       per_sample: bool = False) -> np.ndarray:
        """``X[p, f, j] = sum_n sum_q Hp[n, p, q]^power Y[n, f, q - (A - 1) - m + j]`` with Hp the padded activations of
        ``H`` and ``Y`` a field ``[n, F, *D]`` on the device, float64 ``[P, F, *(A + 2 m)]`` on the host, or per sample
        ``[n, P, F, *(A + 2 m)]`` -> tnmf_hip_triggered_sums.  NotImplementedError for volumes and for a window beyond the
        library's limit."""
        k = len(self.atom_shape)
        if k == 3:
            raise NotImplementedError('triggered sums: 1 or 2 shift axes only')
        assert H.is_cuda and H.dtype == self._torch_dtype and len(margin) == k
        assert Y.is_cuda and Y.dtype == self._torch_dtype and tuple(Y.shape[2:]) == tuple(self._sample_shape)
        assert Y.shape[0] == H.shape[0]
        n, P, F = int(H.shape[0]), int(H.shape[1]), int(Y.shape[1])
        m = (ctypes.c_int * 3)(*[min(int(x), 2 ** 30) for x in margin])
        window = tuple(int(a) + 2 * int(x) for a, x in zip(self.atom_shape, margin))
        # the plan first: it refuses exactly what the call refuses, so nothing is allocated for a window the library does
        # not take (the bytes do not depend on the row stride)
        need = ctypes.c_size_t(0)
        rc = self._lib.tnmf_hip_triggered_sums_plan(self._ctx, ctypes.byref(self._geom(n, P)), F, m, int(bool(per_sample)),
                                                    ctypes.byref(need))
        if rc == _lib.E_UNSUPPORTED:
            raise NotImplementedError(f'triggered sums: a window of {window}, or the number of its sums, is beyond the library\'s limit')
        _lib.check(rc, 'tnmf_hip_triggered_sums_plan')
        X = torch.empty(((n,) if per_sample else ()) + (P, F) + window, dtype=torch.float64, device=self._device)
        if X.numel() == 0:   # (per sample, and no sample)
            return X.cpu().numpy()
        Y = Y.contiguous()
        Hp = self._pad(H)
        work = torch.empty(max(1, need.value), dtype=torch.uint8, device=self._device)
        with self._timed('triggered_sums'):
            self._call_H(Hp, False, lambda Hc, ld: (self._lib.tnmf_hip_triggered_sums(
                self._ctx, ctypes.byref(self._geom(n, P, ld)), _ptr(Hc), _ptr(Y), F, m, int(power), int(bool(per_sample)),
                _ptr(work), need.value, _ptr(X), self._stream()), 'tnmf_hip_triggered_sums'))
        return X.cpu().numpy()

    # -- events: the detections rendered and refitted --------------------------------------------------------------------
    # The H side on a list of events (include/tnmf_hip.h, "events"): no buffer of H's size exists on this path.  The
    # support is fixed over a refit, so the sorted image list and the cell offsets are built once (event_list); only the
    # strengths change between the steps.
    supports_events = True

    def _check_events(self, n_planes: int, sample, plane, shift, strength):
        """-> (sample [K], plane [K], shift [K, k], strength [K]) on the device, checked against this rank's samples, the
        planes of the dictionary and the shift shape of the mode: ValueError for anything out of range, for a strength that
        is negative or not finite; NotImplementedError for volumes."""
        k = len(self.atom_shape)
        if k == 3:
            raise NotImplementedError('events: 1 or 2 shift axes only')

        def dev(x, dtype):
            t = x.to(self._device) if isinstance(x, torch.Tensor) else torch.tensor(np.asarray(x), device=self._device)
            if dtype is torch.int64 and (t.dtype.is_floating_point or t.dtype == torch.bool):
                raise ValueError('events: sample, plane and shift must be integers')
            return t.to(dtype)
        sample, plane = dev(sample, torch.int64).reshape(-1), dev(plane, torch.int64).reshape(-1)
        K = sample.numel()
        shift = dev(shift, torch.int64).reshape(K, k)
        strength = dev(strength, self._torch_dtype).reshape(-1).contiguous()
        if plane.numel() != K or strength.numel() != K:
            raise ValueError('events: sample, plane, shift and strength must have one row per event')
        if K:
            S = torch.tensor(self._transform_shape, dtype=torch.int64, device=self._device)
            bad = torch.stack([((sample < 0) | (sample >= self.n_local_samples)).any(),
                               ((plane < 0) | (plane >= n_planes)).any(), ((shift < 0) | (shift >= S)).any(),
                               (~torch.isfinite(strength) | (strength < 0)).any()]).tolist()
            for flag, what in zip(bad, (f'samples outside [0, {self.n_local_samples})', f'planes outside [0, {n_planes})',
                                        f'shifts outside the shift shape {self._transform_shape}',
                                        'strengths that are negative or not finite')):
                if flag:
                    raise ValueError(f'events: {what}')
        return sample, plane, shift, strength

    def event_list(self, sample: torch.Tensor, plane: torch.Tensor, shift: torch.Tensor):
        """The lists tnmf_hip_events_render / _update take, built on the device for checked events (_check_events):
        (images [I, 4] int32 sorted by (sample, cell), cell_start [cells + 1] int32, events [K, 4] int32).  The images of
        an event per shift axis are ``_Backend.axis_images``; a stable sort keeps, inside a cell, the order image combination,
        then event."""
        k = len(self.atom_shape)
        K = sample.numel()
        mode = self._reconstruction_mode
        with self._timed('event_list'):
            per_axis = []
            for i, (a, s) in enumerate(zip(self.atom_shape, self._transform_shape)):
                first, second, has_second = axis_images(mode, shift[:, i], a, s)
                per_axis.append([(first, None)] + ([] if has_second is None else [(second, has_second)]))
            every = torch.arange(K, dtype=torch.int64, device=self._device)
            es, qs = [], []
            for combo in itertools.product(*per_axis):
                q = torch.stack([c[0] for c in combo], dim=1)
                masks = [c[1] for c in combo if c[1] is not None]
                if not masks:
                    es.append(every)
                    qs.append(q)
                    continue
                sel = torch.nonzero(masks[0] if len(masks) == 1 else masks[0] & masks[1]).reshape(-1)
                es.append(sel)
                qs.append(q[sel])
            e, q = torch.cat(es), torch.cat(qs)
            cells = _lib.EVENT_CELLS[k]
            nc = [-(-(d + a - 1) // c) for d, a, c in zip(self._sample_shape, self.atom_shape, cells)]
            n_keys = self.n_local_samples * int(np.prod(nc))
            if e.numel() >= 2 ** 31 or n_keys >= 2 ** 31 - 1:
                raise NotImplementedError('events: more than 2^31 - 1 images or cells')
            key = sample[e]
            for i in range(k):
                key = key * nc[i] + torch.div(q[:, i], cells[i], rounding_mode='floor')
            key, order = torch.sort(key, stable=True)
            e, q = e[order], q[order]
            zero = torch.zeros_like(e)
            images = torch.stack([plane[e], q[:, 0] if k == 2 else zero, q[:, -1], e], dim=1).to(torch.int32).contiguous()
            cell_start = torch.searchsorted(key, torch.arange(n_keys + 1, dtype=torch.int64, device=self._device)
                                            ).to(torch.int32).contiguous()
            zero = torch.zeros_like(sample)
            events = torch.stack([sample, plane, shift[:, 0] if k == 2 else zero, shift[:, -1]],
                                 dim=1).to(torch.int32).contiguous()
        return images, cell_start, events

    def _events_call(self, name: str, W: torch.Tensor, *args, mode: bool = True) -> None:
        """tnmf_hip_<name>(ctx, the geometry of this rank's samples and the planes of ``W``, the mode when the entry point
        takes one, *args, stream) under the timeline span ``name``."""
        with self._timed(name):
            head = (self._ctx, ctypes.byref(self._geom(self.n_local_samples, W.shape[0]))) + ((self._mode,) if mode else ())
            _lib.check(getattr(self._lib, 'tnmf_hip_' + name)(*head, *args, self._stream()), 'tnmf_hip_' + name)

    def _unweighted_only(self, who: str) -> None:
        if self._G_dev is not None:
            raise NotImplementedError(f'{who} is unweighted')

    def _prepared_events(self, who: Optional[str], n_planes: int, sample, plane, shift, strength,
                         render: Optional[torch.Tensor] = None):
        """What a hook on a list begins with -- the refusal of a weighted fit in the name of ``who`` (None: the hook
        reads no samples), _check_events, event_list -> (images, cell_start, events, strength on the device, R), R the render
        of the list with the dictionary ``render`` (None without one)."""
        if who is not None:
            self._unweighted_only(who)
        sample, plane, shift, strength = self._check_events(n_planes, sample, plane, shift, strength)
        images, cell_start, events = self.event_list(sample, plane, shift)
        R = None if render is None else self.render_event_list(render, images, cell_start, strength)
        return images, cell_start, events, strength, R

    def _new_ab_mag(self, shape, with_magnitude: bool):
        """(a, b, mag): float64 outputs of ``shape`` on the device, mag None unless asked for."""
        a, b = (torch.empty(shape, dtype=torch.float64, device=self._device) for _ in range(2))
        return a, b, torch.empty(shape, dtype=torch.float64, device=self._device) if with_magnitude else None

    def render_event_list(self, W: torch.Tensor, images: torch.Tensor, cell_start: torch.Tensor, strength: torch.Tensor,
                          R: Optional[torch.Tensor] = None) -> torch.Tensor:
        """R[n_local, C, *D] of the image list (event_list) and the strengths -> tnmf_hip_events_render (into R when
        given: every element is written)."""
        self._check_W(W)
        assert strength.is_cuda and strength.is_contiguous() and strength.dtype == self._torch_dtype
        shape = (self.n_local_samples, self.n_channels) + self._sample_shape
        if R is None:
            R = torch.empty(shape, dtype=self._torch_dtype, device=self._device)
        assert R.is_contiguous() and tuple(R.shape) == shape and R.dtype == self._torch_dtype
        self._events_call('events_render', W, _ptr(W), _ptr(images), images.shape[0], _ptr(cell_start), _ptr(strength),
                          strength.numel(), _ptr(R), mode=False)
        return R

    def update_event_list(self, W: torch.Tensor, events: torch.Tensor, strength: torch.Tensor, R: torch.Tensor,
                          sparsity: float = 0., eps: float = 1e-9) -> None:
        """One multiplicative update of the strengths in place, R being their render -> tnmf_hip_events_update."""
        self._check_W(W)
        assert strength.is_contiguous() and strength.dtype == self._torch_dtype and events.shape[0] == strength.numel()
        self._events_call('events_update', W, _ptr(W), _ptr(events), _ptr(strength), strength.numel(), _ptr(self._V_dev),
                          _ptr(R), float(eps), float(sparsity))

    def render_events(self, W: torch.Tensor, sample, plane, shift, strength) -> torch.Tensor:
        """R[n_local, C, *D]: what the events (local sample, plane of W, shift in H of this mode, strength) reconstruct --
        the reconstruction of the activations that hold the strengths at the events and zero elsewhere, without those
        activations.  Duplicate events add up."""
        return self._prepared_events(None, W.shape[0], sample, plane, shift, strength, render=W)[-1]

    def refit_events(self, V, W: torch.Tensor, sample, plane, shift, strength, n_iterations: int, sparsity: float = 0.,
                     eps: float = 1e-9) -> torch.Tensor:
        """[K] strengths after ``n_iterations`` multiplicative updates on the fixed support, W fixed, against the resident
        samples (`V` is the array given to initialize(), as for the other hooks): per step one render and one update.
        The plain Frobenius objective; the events must be distinct in (sample, plane, shift)."""
        images, cell_start, events, strength, _ = self._prepared_events('refit_events', W.shape[0], sample, plane, shift,
                                                                        strength)
        strength = strength.clone()
        R = torch.empty_like(self._V_dev)
        for _ in range(int(n_iterations)):
            self.render_event_list(W, images, cell_start, strength, R)
            self.update_event_list(W, events, strength, R, sparsity, eps)
        return strength

    def gain_event_list(self, W: torch.Tensor, events: torch.Tensor, strength: torch.Tensor, R: torch.Tensor,
                        with_magnitude: bool = False):
        """[K] float64 on the device: what each event explains, R being the render of the strengths ->
        tnmf_hip_events_gain; with ``with_magnitude`` (gain, mag), mag the sum of the magnitudes of each gain's terms."""
        self._check_W(W)
        assert strength.is_contiguous() and strength.dtype == self._torch_dtype and events.shape[0] == strength.numel()
        K = strength.numel()
        gain = torch.empty(K, dtype=torch.float64, device=self._device)
        mag = torch.empty(K, dtype=torch.float64, device=self._device) if with_magnitude else None
        self._events_call('events_gain', W, _ptr(W), _ptr(events), _ptr(strength), K, _ptr(self._V_dev), _ptr(R), _ptr(gain),
                          _ptr(mag))
        return (gain, mag) if with_magnitude else gain

    def event_gains(self, V, W: torch.Tensor, sample, plane, shift, strength) -> np.ndarray:
        """[K] float64 on the host: per event the Frobenius energy of the list without it minus that of the list, against
        the resident samples (`V` is the array given to initialize(), as for the other hooks): one render of the list and
        one gather per event; only the K doubles are copied.  Duplicate events are scored each against the whole list."""
        _, _, events, strength, R = self._prepared_events('event_gains', W.shape[0], sample, plane, shift, strength, render=W)
        return self.gain_event_list(W, events, strength, R).cpu().numpy()

    def landscape_event_list(self, W: torch.Tensor, events: torch.Tensor, strength: torch.Tensor, R: torch.Tensor,
                             with_magnitude: bool = False):
        """(a, b) [K, 3^k] float64 on the device: every event at its neighbouring shifts against the residual of the list
        without it, R being the render of the strengths -> tnmf_hip_events_landscape; with ``with_magnitude`` (a, b, mag),
        mag the sum of the magnitudes of the terms of a."""
        self._check_W(W)
        assert strength.is_contiguous() and strength.dtype == self._torch_dtype and events.shape[0] == strength.numel()
        assert R.is_contiguous() and R.dtype == self._torch_dtype and tuple(R.shape) == tuple(self._V_dev.shape)
        K = strength.numel()
        a, b, mag = self._new_ab_mag((K, 3 ** len(self.atom_shape)), with_magnitude)
        self._events_call('events_landscape', W, _ptr(W), _ptr(events), _ptr(strength), K, _ptr(self._V_dev), _ptr(R),
                          _ptr(a), _ptr(b), _ptr(mag))
        return (a, b, mag) if with_magnitude else (a, b)

    def event_landscape(self, V, W: torch.Tensor, sample, plane, shift, strength):
        """(a, b) [K, 3^k] float64 on the host: per event and neighbouring shift the correlation of the occurrence there
        with the residual of the list without the event, and its norm, against the resident samples (`V` is the array given
        to initialize(), as for the other hooks): one render of the list and one kernel; only the 2 * K * 3^k doubles are
        copied.  Duplicate events put back only themselves."""
        _, _, events, strength, R = self._prepared_events('event_landscape', W.shape[0], sample, plane, shift, strength,
                                                          render=W)
        a, b = self.landscape_event_list(W, events, strength, R)
        return a.cpu().numpy(), b.cpu().numpy()

    def alternatives_event_list(self, W: torch.Tensor, events: torch.Tensor, strength: torch.Tensor, R: torch.Tensor,
                                n_alt: int, stride: int, with_magnitude: bool = False):
        """(a, b) [K, n_alt] float64 on the device: every event under the planes ``first + j * stride`` of its block of
        ``n_alt * stride`` planes, at its own shift, against the residual of the list without it, R being the render of the
        strengths -> tnmf_hip_events_alternatives; with ``with_magnitude`` (a, b, mag), mag the sum of the magnitudes of the
        terms of a."""
        self._check_W(W)
        assert strength.is_contiguous() and strength.dtype == self._torch_dtype and events.shape[0] == strength.numel()
        assert R.is_contiguous() and R.dtype == self._torch_dtype and tuple(R.shape) == tuple(self._V_dev.shape)
        K, n_alt, stride = strength.numel(), int(n_alt), int(stride)
        a, b, mag = self._new_ab_mag((K, max(n_alt, 0)), with_magnitude)
        self._events_call('events_alternatives', W, _ptr(W), _ptr(events), _ptr(strength), K, _ptr(self._V_dev), _ptr(R),
                          n_alt, stride, _ptr(a), _ptr(b), _ptr(mag))
        return (a, b, mag) if with_magnitude else (a, b)

    def event_alternatives(self, V, W: torch.Tensor, sample, plane, shift, strength, n_alt: int, stride: int):
        """(a, b) [K, n_alt] float64 on the host: per event and candidate plane the correlation of that plane's occurrence
        at the event's shift with the residual of the list without the event, and its norm, against the resident samples
        (`V` is the array given to initialize(), as for the other hooks): one render of the list and one kernel; only the
        2 * K * n_alt doubles are copied.  Duplicate events put back only themselves."""
        _, _, events, strength, R = self._prepared_events('event_alternatives', W.shape[0], sample, plane, shift, strength,
                                                          render=W)
        a, b = self.alternatives_event_list(W, events, strength, R, n_alt, stride)
        return a.cpu().numpy(), b.cpu().numpy()

    # -- events: the patches under the rows and their moments per atom ---------------------------------------------------------
    # The data under each row, gathered where the samples live (include/tnmf_hip.h, "patches"); the moments of a long list
    # are taken chunk by chunk through one reused buffer, so neither K * D doubles nor V cross to the host.
    PATCH_BYTES = 256 << 20      # the patches of one chunk of event_patch_moments: at most this much

    def patch_event_list(self, W: Optional[torch.Tensor], events: torch.Tensor, strength: torch.Tensor,
                         R: Optional[torch.Tensor], source: str, table, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[K, C, *A] float64 on the device: the patch of every row, R being the render of the strengths (None for
        ``source='data'``), folded into the atom frame by ``table`` (_fold_table; (None, None, None, 1): the image frame)
        -> tnmf_hip_events_patches (into the first K rows of ``out`` when given: every element is written)."""
        assert strength.is_contiguous() and strength.dtype == self._torch_dtype and events.shape[0] == strength.numel()
        assert events.is_contiguous() and (R is None) == (source == 'data')
        K = strength.numel()
        shape = (K, self.n_channels) + tuple(self.atom_shape)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=self._device)
        assert out.is_contiguous() and out.dtype == torch.float64 and out.numel() >= int(np.prod(shape))
        ptr, src, w, T = table
        # (the table's length is not an operand of the entry: the caller vouches that it is the one of this atom shape)
        assert ptr is None or (ptr.numel() == T * int(np.prod(self.atom_shape)) + 1 and src.numel() == w.numel())
        n_planes = T if W is None else W.shape[0]
        with self._timed('events_patches'):
            _lib.check(self._lib.tnmf_hip_events_patches(
                self._ctx, ctypes.byref(self._geom(self.n_local_samples, n_planes)), self._mode, _lib.PATCH_SOURCES[source],
                _ptr(W), _ptr(events), _ptr(strength), K, _ptr(self._V_dev), _ptr(R), _ptr(ptr), _ptr(src), _ptr(w), T,
                _ptr(out), self._stream()), 'tnmf_hip_events_patches')
        return out.reshape(-1)[:int(np.prod(shape))].reshape(shape)

    def event_patches(self, V, W: torch.Tensor, sample, plane, shift, strength, source: str = 'cleaned', transforms=None,
                      frame: str = 'atom') -> np.ndarray:
        """[K, C, *A] float64 on the host: the data under each row of the list, against the resident samples (`V` is the
        array given to initialize(), as for the other hooks) -- ``source`` 'data': V, 'residual': V - R, 'cleaned':
        V - R + h phi -- in the frame of the plane (``frame='image'``) or folded by the transposed operator of the row's
        transform into the frame of the atom (``'atom'``).  The list is rendered only when the source needs R."""
        self._check_W(W)
        _, _, events, strength, R = self._prepared_events('event_patches', W.shape[0], sample, plane, shift, strength,
                                                          render=None if source == 'data' else W)
        table = self._fold_table(transforms if frame == 'atom' else None)
        if W.shape[0] % table[3]:
            raise ValueError(f'event_patches: {W.shape[0]} planes are not a multiple of the {table[3]} transforms')
        return self.patch_event_list(W, events, strength, R, source, table).cpu().numpy()

    def moments_patch_list(self, Y: torch.Tensor, strength_d: torch.Tensor, by_atom: torch.Tensor, atom_start: torch.Tensor,
                           n_rows: int, accumulate: bool, out) -> None:
        """The moments (S [M, D, D], g [M, D], s2 [M], count [M]) = ``out`` of the first ``n_rows`` rows of ``Y[., D]``,
        written or (``accumulate``) added to -> tnmf_hip_patch_moments."""
        S, g, s2, count = out
        M, D = g.shape
        assert all(t.is_contiguous() and t.dtype == torch.float64 for t in (Y, strength_d, S, g, s2, count))
        assert by_atom.dtype == torch.int32 and atom_start.dtype == torch.int32 and atom_start.numel() == M + 1
        assert Y.numel() >= n_rows * D and strength_d.numel() >= n_rows and by_atom.numel() >= n_rows
        with self._timed('patch_moments'):
            _lib.check(self._lib.tnmf_hip_patch_moments(
                self._ctx, D, M, _ptr(Y), _ptr(strength_d), _ptr(by_atom), _ptr(atom_start), n_rows, 1 if accumulate else 0,
                _ptr(S), _ptr(g), _ptr(s2), _ptr(count), self._stream()), 'tnmf_hip_patch_moments')

    def patch_chunk_rows(self, max_rows: Optional[int] = None) -> int:
        """The rows of one chunk of event_patch_moments: ``max_rows`` (default: what keeps the patches within PATCH_BYTES)
        rounded down to a multiple of _lib.EVENT_SEGMENT, and at least that."""
        D = self.n_channels * int(np.prod(self.atom_shape))
        rows = self.PATCH_BYTES // (8 * D) if max_rows is None else int(max_rows)
        return max(rows // _lib.EVENT_SEGMENT, 1) * _lib.EVENT_SEGMENT

    def event_patch_moments(self, V, W: torch.Tensor, sample, plane, shift, strength, source: str = 'cleaned',
                            transforms=None, max_rows: Optional[int] = None):
        """(S [M, D, D], g [M, D], s2 [M], count [M]) float64 on the host, M = planes / T atoms and D = C * prod(A): per atom
        the second moments of the atom-frame patches of its rows, ``S = sum y y^T``, ``g = sum h y``, ``s2 = sum h^2``, the
        rows of an atom in list order.  The list is sorted by atom (stable) and walked in chunks of ``patch_chunk_rows``
        rows: the patches of a chunk into one reused buffer, then their moments added to the outputs.  The chunks depend
        on K, D and ``max_rows`` alone and begin at multiples of four rows, where tnmf_hip_patch_moments continues the
        bits: the result does not depend on ``max_rows``."""
        self._check_W(W)
        _, _, events, strength, R = self._prepared_events('event_patch_moments', W.shape[0], sample, plane, shift, strength,
                                                          render=None if source == 'data' else W)
        table = self._fold_table(transforms)
        T = table[3]
        if W.shape[0] % T:
            raise ValueError(f'event_patch_moments: {W.shape[0]} planes are not a multiple of the {T} transforms')
        M, K = W.shape[0] // T, strength.numel()
        D = self.n_channels * int(np.prod(self.atom_shape))
        if M * D * D >= 2 ** 31:
            raise NotImplementedError('event_patch_moments: more than 2^31 - 1 entries of S')
        with self._timed('event_atom_list'):
            sorted_atom, order = torch.sort(torch.div(events[:, 1].to(torch.int64), T, rounding_mode='floor'), stable=True)
            atom_start = torch.searchsorted(sorted_atom, torch.arange(M + 1, dtype=torch.int64, device=self._device))
            events, strength = events[order].contiguous(), strength[order].contiguous()
            strength_d = strength.to(torch.float64)
        chunk = self.patch_chunk_rows(max_rows)
        Y = torch.empty((min(chunk, K), D), dtype=torch.float64, device=self._device)
        by_atom = torch.arange(min(chunk, K), dtype=torch.int32, device=self._device)
        out = (torch.empty((M, D, D), dtype=torch.float64, device=self._device),
               torch.empty((M, D), dtype=torch.float64, device=self._device),
               torch.empty(M, dtype=torch.float64, device=self._device),
               torch.empty(M, dtype=torch.float64, device=self._device))
        for r0 in range(0, max(K, 1), chunk):      # (without rows: one call that writes the zeros)
            n = min(chunk, K - r0)
            self.patch_event_list(W, events[r0:r0 + n], strength[r0:r0 + n], R, source, table, out=Y)
            self.moments_patch_list(Y, strength_d[r0:r0 + n], by_atom, (atom_start - r0).clamp(0, n).to(torch.int32), n,
                                    r0 > 0, out)
        return tuple(t.cpu().numpy() for t in out)

    # -- events: exact strengths ---------------------------------------------------------------------------------------------
    # The objective of a list is a quadratic in its strengths (include/tnmf_hip.h, "events: exact strengths"): the samples
    # enter once, through c = <phi, V>; the solver then works on K-vectors and the non-zeros of the Gram matrix alone.
    def gram_event_list(self, W: torch.Tensor, images: torch.Tensor, cell_start: torch.Tensor, events: torch.Tensor,
                        capacity: Optional[int] = None):
        """(row_start [K + 1] int32, col [nnz] int32, val [nnz] float64) on the device: the Gram matrix G_ij = <phi_i, phi_j> of
        the rows ``events`` (event_list) in CSR, columns ascending, the diagonal present, bit-symmetric ->
        tnmf_hip_events_pairs (sized by a guess, ``capacity``; once more with the count when it did not fit), the pairs
        made unique and ordered here, tnmf_hip_events_gram on i <= j, the values mirrored.  The timeline books the two
        kernels alone ('events_pairs', 'events_gram') and the torch work on the lists under 'events_gram_lists'."""
        self._check_W(W)
        K = int(events.shape[0])
        every = torch.arange(K, dtype=torch.int64, device=self._device)
        count = torch.zeros(1, dtype=torch.int64, device=self._device)
        cap = max(4096, 16 * int(images.shape[0])) if capacity is None else int(capacity)
        for _ in range(2):   # a guess, and once more with the count when it did not fit
            keys = torch.empty(cap, dtype=torch.int64, device=self._device)
            self._events_call('events_pairs', W, _ptr(images), images.shape[0], _ptr(cell_start), _ptr(events), K, _ptr(keys),
                              cap, _ptr(count), mode=False)
            total = int(count.item())
            if total <= cap:
                break
            cap = total
        assert total <= cap, 'the same lists give the same count'
        with self._timed('events_gram_lists'):
            upper = torch.unique(keys[:total])            # sorted: i * K + j, i < j
            upper = torch.cat([every * K + every, upper])  # the diagonal first, then the rows above it
            ri = torch.div(upper, max(K, 1), rounding_mode='floor')
            rj = upper - ri * K
            ri32, rj32 = ri.to(torch.int32).contiguous(), rj.to(torch.int32).contiguous()
            val = torch.empty(upper.numel(), dtype=torch.float64, device=self._device)
        self._events_call('events_gram', W, _ptr(W), _ptr(events), K, _ptr(ri32), _ptr(rj32), upper.numel(), _ptr(val))
        with self._timed('events_gram_lists'):
            # both triangles from the one value of a pair; a candidate whose value is exactly 0 is dropped
            live = val[K:] != 0
            ui, uj, uv = ri[K:][live], rj[K:][live], val[K:][live]
            key = torch.cat([upper[:K], ui * K + uj, uj * K + ui])
            key, order = torch.sort(key)
            v = torch.cat([val[:K], uv, uv])[order].contiguous()
            row = torch.div(key, max(K, 1), rounding_mode='floor')
            col = (key - row * K).to(torch.int32).contiguous()
            row_start = torch.searchsorted(row, torch.arange(K + 1, dtype=torch.int64, device=self._device)
                                           ).to(torch.int32).contiguous()
        if v.numel() >= 2 ** 31:
            raise NotImplementedError('events: more than 2^31 - 1 entries in the Gram matrix')
        return row_start, col, v

    def project_event_list(self, W: torch.Tensor, events: torch.Tensor) -> torch.Tensor:
        """c [K] float64 on the device: <phi_e, V> of every row against the resident samples -> tnmf_hip_events_project."""
        self._check_W(W)
        K = int(events.shape[0])
        c = torch.empty(K, dtype=torch.float64, device=self._device)
        self._events_call('events_project', W, _ptr(W), _ptr(events), K, _ptr(self._V_dev), _ptr(c))
        return c

    def nnls_event_list(self, csr, c: torch.Tensor, start: torch.Tensor, tol: float, max_iterations: int,
                        check_every: int = 10):
        """(h [K] float64 on the device, info): min 1/2 h'Gh - c'h over h >= 0 from ``start`` projected ->
        tnmf_hip_events_nnls; info: iterations, kkt, converged, nnz, history [checks, 2]."""
        row_start, col, val = csr
        K = c.numel()
        assert row_start.dtype == torch.int32 and col.dtype == torch.int32 and val.dtype == torch.float64
        assert c.dtype == torch.float64 and row_start.numel() == K + 1 and col.numel() == val.numel()
        h = start.to(torch.float64).reshape(-1).clone().contiguous()
        assert h.numel() == K
        ws = torch.empty(7 * K + 8, dtype=torch.float64, device=self._device)
        cap = int(max_iterations) // int(check_every) + 2
        history = np.zeros((cap, 2), dtype=np.float64)
        it, conv, nh, kkt = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0.)
        with self._timed('events_nnls'):
            _lib.check(self._lib.tnmf_hip_events_nnls(
                self._ctx, K, val.numel(), _ptr(row_start), _ptr(col), _ptr(val), _ptr(c), _ptr(h), float(tol),
                int(max_iterations), int(check_every), _ptr(ws), ctypes.byref(it), ctypes.byref(kkt), ctypes.byref(conv),
                history.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cap, ctypes.byref(nh), self._stream()),
                'tnmf_hip_events_nnls')
        return h, dict(iterations=int(it.value), kkt=float(kkt.value), converged=bool(conv.value), nnz=int(val.numel()),
                       history=history[:nh.value].copy())

    def solve_events(self, V, W: torch.Tensor, sample, plane, shift, strength, tol: float, max_iterations: int,
                     check_every: int = 10):
        """(strength [K] float64 on the device, info): the strengths that minimise the plain Frobenius objective on the
        fixed support, against the resident samples (`V` is the array given to initialize(), as for the other hooks), from
        the given ones: the lists, the Gram matrix, the projection, the solver -- no render of the sample frame.  info:
        iterations, kkt, converged, nnz, history [checks, 2] (iteration, kkt).  The events must be distinct.  With a process
        group every rank solves its own samples: rows of different samples never couple, so there is no collective."""
        images, cell_start, events, strength, _ = self._prepared_events('solve_events', W.shape[0], sample, plane, shift,
                                                                        strength)
        csr = self.gram_event_list(W, images, cell_start, events)
        c = self.project_event_list(W, events)
        return self.nnls_event_list(csr, c, strength, tol, max_iterations, check_every)

    # -- events: standard errors ---------------------------------------------------------------------------------------------
    # Cov(h_A) = sigma^2 (G_AA)^-1 on the active rows A (include/tnmf_hip.h, "events: standard errors"): G_AA is block diagonal
    # over the connected components of its coupling graph, found here on the device; the kernel inverts each block.
    def _csr_rows(self, csr) -> torch.Tensor:
        """row [nnz] int64: the row of every stored entry."""
        row_start, col, _ = csr
        K = row_start.numel() - 1
        return torch.repeat_interleave(torch.arange(K, dtype=torch.int64, device=self._device),
                                       (row_start[1:] - row_start[:-1]).to(torch.int64), output_size=col.numel())

    def event_components(self, csr, active: torch.Tensor):
        """The connected components of the graph of ``csr`` (gram_event_list) restricted to the entries whose row and column
        are both ``active`` ([K] bool on the device) -> dict(comp_start [n_comp + 1] int32, member [K_A] int32: the active
        rows grouped by component and ascending inside each, local [K] int32: a row's position inside its component, -1 for
        a row that is not active, row_size [K] int64: the size of a row's component, 0 where not active -- all on the device
        -- and on the host sizes [n_comp] int32 and rounds).  The components come in ascending size, equal sizes by their
        smallest row.  Labels by min-label hooking with pointer jumping: in a round the root of every tree takes the
        smallest label its members see across an edge, then ceil(log2 K) jumps label <- label[label] flatten the trees
        again; a round halves the trees that can still merge, where plain propagation moves a label one edge.  The host reads
        one flag per round, the counts of the result, and no array of the size of the matrix."""
        row_start, col, _ = csr
        K = int(row_start.numel()) - 1
        with self._timed('events_components'):
            active = active.to(device=self._device, dtype=torch.bool).reshape(-1)
            assert active.numel() == K
            every = torch.arange(K, dtype=torch.int64, device=self._device)
            label, rounds = every, 0
            if col.numel() > K:   # (the diagonal alone: no edges)
                u, c = self._csr_rows(csr), col.to(torch.int64)
                v = torch.where(active[u] & active[c], c, u)   # (an entry that is no edge of the graph: a loop at its row)
                jumps = max(1, (K - 1).bit_length())
                while True:
                    rounds += 1
                    new = label.scatter_reduce(0, label[u], label[v], 'amin', include_self=True)
                    for _ in range(jumps):
                        new = new[new]
                    changed = bool((new != label).any())   # the one scalar of the round
                    label = new
                    if not changed:
                        break
            rows = torch.nonzero(active).reshape(-1)
            roots, which, counts = torch.unique(label[rows], return_inverse=True, return_counts=True)
            order = torch.argsort(counts * (K + 1) + roots)         # ascending size, then the smallest row
            rank = torch.empty_like(order)
            rank[order] = torch.arange(order.numel(), dtype=torch.int64, device=self._device)
            comp = rank[which]                                      # the component of every active row
            by_comp = torch.argsort(comp * max(K, 1) + rows)
            member, comp = rows[by_comp], comp[by_comp]
            sizes = counts[order]
            comp_start = torch.cat([torch.zeros(1, dtype=torch.int64, device=self._device), torch.cumsum(sizes, 0)])
            local = torch.full((K,), -1, dtype=torch.int64, device=self._device)
            local[member] = torch.arange(member.numel(), dtype=torch.int64, device=self._device) - comp_start[comp]
            row_size = torch.zeros(K, dtype=torch.int64, device=self._device)
            row_size[member] = sizes[comp]
            return dict(comp_start=comp_start.to(torch.int32).contiguous(), member=member.to(torch.int32).contiguous(),
                        local=local.to(torch.int32).contiguous(), row_size=row_size,
                        sizes=np.ascontiguousarray(sizes.cpu().numpy().astype(np.int32)), rounds=rounds)

    def inverse_diag_event_list(self, csr, active: torch.Tensor, max_component: int = 2048,
                                out: Optional[torch.Tensor] = None, scratch_doubles: Optional[int] = None):
        """(d [K] float64 on the device, info): d_i = ((G_AA)^-1)_ii for the rows of ``active``, NaN for the others, +inf
        for the rows of a component that is numerically singular -> event_components, tnmf_hip_events_inverse_diag.
        ValueError, before ``out`` (d, when given) is written, for a component of more than ``max_component`` rows.  info:
        n_active, n_components, largest_component, n_singular, rounds, sizes [n_comp] and status [n_comp] on the host,
        row_size [K] on the device.  ``scratch_doubles``: the scratch of the components beyond the LDS path (default: what
        they all take, at most 2^24 doubles or one tile of the largest)."""
        row_start, col, val = csr
        K = int(row_start.numel()) - 1
        assert row_start.dtype == torch.int32 and col.dtype == torch.int32 and val.dtype == torch.float64
        comps = self.event_components(csr, active)
        sizes = comps['sizes']
        largest = int(sizes[-1]) if len(sizes) else 0
        if largest > int(max_component):
            raise ValueError(f'events: the largest component of the active rows has {largest} rows, more than '
                             f'max_component={int(max_component)}')
        d = torch.empty(K, dtype=torch.float64, device=self._device) if out is None else out
        assert d.dtype == torch.float64 and d.is_contiguous() and d.numel() == K
        tiles = [int(n) * int(n) + int(n) for n in sizes if n > _lib.EVENT_INVERSE_LDS]
        if scratch_doubles is None:
            scratch_doubles = min(sum(tiles), max(2 ** 24, tiles[-1])) if tiles else 0
        scratch = torch.empty(int(scratch_doubles), dtype=torch.float64, device=self._device)
        status = torch.zeros(len(sizes), dtype=torch.int32, device=self._device)
        args = (self._ctx, K, val.numel(), _ptr(row_start), _ptr(col), _ptr(val), len(sizes), _ptr(comps['comp_start']),
                sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), comps['member'].numel(), _ptr(comps['member']),
                _ptr(comps['local']), _ptr(scratch) if scratch.numel() else None, scratch.numel(), _ptr(d), _ptr(status),
                self._stream())
        with self._timed('events_inverse_diag'):
            code = self._lib.tnmf_hip_events_inverse_diag(*args)
        _lib.check(code, 'tnmf_hip_events_inverse_diag')
        status = status.cpu().numpy()
        return d, dict(n_active=int(comps['member'].numel()), n_components=len(sizes), largest_component=largest,
                       n_singular=int(np.count_nonzero(status)), rounds=int(comps['rounds']), sizes=sizes, status=status,
                       row_size=comps['row_size'])

    def event_errors(self, V, W: torch.Tensor, sample, plane, shift, strength, max_component: int = 2048):
        """(d [K], b [K], residual energy, info) for the standard errors of the strengths of a list against the resident
        samples (`V` is the array given to initialize(), as for the other hooks): with A the rows of strength > 0,
        d = diag (G_AA)^-1 (inverse_diag_event_list: NaN off A, +inf on a singular component), b = diag G, and
        ||V - R(list)||^2 = ||V||^2 - 2 c'h + h'Gh in double from c, G, h and the samples' own energy -- no render --, not
        below 0.  d and b are float64 on the device, the energy a float.  The events must be distinct.  With a process
        group every rank takes its own samples: there is no collective."""
        images, cell_start, events, strength, _ = self._prepared_events('event_errors', W.shape[0], sample, plane, shift,
                                                                        strength)
        csr = self.gram_event_list(W, images, cell_start, events)
        c = self.project_event_list(W, events)
        h = strength.to(torch.float64)
        d, info = self.inverse_diag_event_list(csr, h > 0, max_component)
        K = h.numel()
        row, col, val = self._csr_rows(csr), csr[1].to(torch.int64), csr[2]
        b = torch.zeros(K, dtype=torch.float64, device=self._device)
        on_diagonal = row == col
        b[row[on_diagonal]] = val[on_diagonal]
        v = self._V_dev.to(torch.float64)
        energy = torch.sum(v * v) - 2. * torch.sum(c * h) + torch.sum(val * h[row] * h[col])
        return d, b, max(float(energy), 0.), info

    # -- pursuit: the list found by forward selection ---------------------------------------------------------------------
    # A round (include/tnmf_hip.h, "pursuit") is the H gradient's numerator of the residual, the gain map, its peaks and
    # the exact score of the kept ones; the rows are chosen on the host (events_host.pursuit_loop) from the
    # peaks alone -- the map, activation-sized, never leaves the device.
    def event_norms(self, W: torch.Tensor) -> torch.Tensor:
        """b[P, *S] float64 on the device: ||phi||^2 of every plane of ``W`` at every shift of this mode ->
        tnmf_hip_events_norms."""
        self._check_W(W)
        if len(self.atom_shape) == 3:
            raise NotImplementedError('events: 1 or 2 shift axes only')
        b = torch.empty((W.shape[0],) + self._transform_shape, dtype=torch.float64, device=self._device)
        self._events_call('events_norms', W, _ptr(W), _ptr(b))
        return b

    def pursuit_buffers(self, n_planes: int):
        """The activation-sized work arrays of a pursuit, allocated once for all its rounds: (neg, pos) of the padded shape
        for tnmf_hip_grad_H and, in a mode that folds, the map of the mode's shift shape (else None: neg is the map)."""
        shape = (self.n_local_samples, n_planes)
        neg = torch.empty(shape + self._padded_shape, dtype=self._torch_dtype, device=self._device)
        pos = torch.empty_like(neg)
        folded = None if self._mode == 0 else torch.empty(shape + self._transform_shape, dtype=self._torch_dtype,
                                                          device=self._device)
        return neg, pos, folded

    def _correlate_residual(self, W: torch.Tensor, d: torch.Tensor, buffers=None) -> torch.Tensor:
        """a[n, P, *S]: the correlation of the residual ``d[n, C, *D]`` with every plane of W, folded for the mode -- the
        numerator of tnmf_hip_grad_H with d in the place of the samples (and of R: the second output is not used), written
        into ``buffers`` (pursuit_buffers; made here when not given).  The FFT family may keep the spectra of the samples it
        is given by pointer; d changes every round at the same address, so whatever the library holds is dropped before the
        call, and after it, when it describes d and not the fit."""
        n, P = d.shape[0], W.shape[0]
        neg, pos, folded = self.pursuit_buffers(P) if buffers is None else buffers
        assert tuple(neg.shape) == (n, P) + self._padded_shape and neg.is_contiguous() and pos.shape == neg.shape
        self._foreign_H()
        try:
            with self._timed('pursuit_correlate'):
                _lib.check(self._lib.tnmf_hip_grad_H(self._ctx, ctypes.byref(self._geom(n, P)), _ptr(d), _ptr(d), _ptr(W),
                                                     None, _ptr(neg), _ptr(pos), self._stream()), 'tnmf_hip_grad_H')
        finally:
            self._foreign_H()
        if folded is None:
            return neg
        _lib.check(self._lib.tnmf_hip_fold_H(self._ctx, ctypes.byref(self._geom(n, P)), self._mode, _ptr(neg), _ptr(folded),
                                             self._stream()), 'tnmf_hip_fold_H')
        return folded

    def pursuit_round(self, W: torch.Tensor, b: torch.Tensor, d: torch.Tensor, taken: torch.Tensor, min_gain: float,
                      buffers=None) -> Tuple[np.ndarray, np.ndarray]:
        """(idx, val) on the host: the candidates of a round -- the peaks above ``min_gain``, within ``atom_shape - 1`` over
        all planes, of the gain map ``a^2 / (2 b)`` of the residual ``d`` with the entries ``taken`` (int64 flat indices, the
        rows of the list) zeroed -> tnmf_hip_grad_H, tnmf_hip_pursuit_score (in place on the map), tnmf_hip_find_peaks."""
        k = len(self.atom_shape)
        a = self._correlate_residual(W, d, buffers)
        assert a.is_contiguous() and tuple(a.shape[1:]) == tuple(b.shape) and b.dtype == torch.float64
        assert taken.dtype == torch.int64 and taken.is_contiguous()
        g = _lib.make_geom(int(a.shape[0]), int(a.shape[1]), self.n_channels, tuple(a.shape[2:]), (1,) * k,
                           self._dtype_code, 0)
        with self._timed('pursuit_score'):
            _lib.check(self._lib.tnmf_hip_pursuit_score(self._ctx, ctypes.byref(g), _ptr(a), _ptr(b), _ptr(a), _ptr(taken),
                                                        taken.numel(), self._stream()), 'tnmf_hip_pursuit_score')
        return self.find_peaks(a, float(min_gain), tuple(x - 1 for x in self.atom_shape), int(a.shape[1]))

    def pick_events(self, W: torch.Tensor, idx: torch.Tensor, R: torch.Tensor, with_magnitude: bool = False):
        """(events [K, 4] int32, strength [K], gain [K] float64) on the device for the flat indices ``idx`` (int64) in
        [n_local, P, *S]: the rows, their best strengths against the residual of the render R and what adding them gains,
        summed in double -> tnmf_hip_pursuit_pick; with ``with_magnitude`` also mag, the scale of the rounding error."""
        self._check_W(W)
        assert idx.dtype == torch.int64 and idx.is_contiguous() and R.is_contiguous() and R.dtype == self._torch_dtype
        assert tuple(R.shape) == tuple(self._V_dev.shape)
        K = idx.numel()
        events = torch.empty((K, 4), dtype=torch.int32, device=self._device)
        strength = torch.empty(K, dtype=self._torch_dtype, device=self._device)
        gain = torch.empty(K, dtype=torch.float64, device=self._device)
        mag = torch.empty(K, dtype=torch.float64, device=self._device) if with_magnitude else None
        self._events_call('pursuit_pick', W, _ptr(W), _ptr(idx), K, _ptr(self._V_dev), _ptr(R), _ptr(events), _ptr(strength),
                          _ptr(gain), _ptr(mag))
        return (events, strength, gain, mag) if with_magnitude else (events, strength, gain)

    def pursue_events(self, V, W: torch.Tensor, sample, plane, shift, strength, min_gain: float,
                      max_events: Optional[int] = None, max_rounds: int = 100, refit_iterations: int = 10,
                      eps: float = 1e-9, solve: Optional[Tuple[float, int]] = None):
        """(sample, plane, shift, strength, history) on the host: the list (this rank's local samples) grown from the given
        one by forward selection against the resident samples (`V` is the array given to initialize(), as for the other
        hooks) -- per round one render of the list, the residual, pursuit_round, the host's choice among the candidates,
        pick_events for the kept ones and refit_events for the list; only candidates and kept rows cross to the host.  The
        resident samples and the model's activations are left as they are.  The plain Frobenius objective.  With
        ``solve = (tol, max_iterations)`` the list's strengths of a round are solve_events', not refit_events'."""
        self._unweighted_only('pursue_events')
        P, k = int(W.shape[0]), len(self.atom_shape)
        sample, plane, shift, strength = self._check_events(P, sample, plane, shift, strength)
        b = self.event_norms(W)
        R, d = torch.empty_like(self._V_dev), torch.empty_like(self._V_dev)
        buffers = self.pursuit_buffers(P)   # (activation-sized: once for all the rounds)
        shape = (self.n_local_samples, P) + self._transform_shape

        def candidates(sample, plane, shift, strength):
            s, p, u, h = self._check_events(P, sample, plane, shift, strength)
            if s.numel():
                images, cell_start, _ = self.event_list(s, p, u)
                self.render_event_list(W, images, cell_start, h, R)
            else:
                R.zero_()
            d.copy_(R)      # d = V - R, rounded once
            _lib.check(self._lib.tnmf_hip_axpby(self._ctx, self._dtype_code, _ptr(d), _ptr(self._V_dev), -1., 1., d.numel(),
                                                self._stream()), 'tnmf_hip_axpby')
            taken = s * P + p
            for i in range(k):
                taken = taken * self._transform_shape[i] + u[:, i]
            return self.pursuit_round(W, b, d, taken.contiguous(), min_gain, buffers)

        def score(sample, plane, shift, strength, idx):   # (R is the render of this list: candidates() came first)
            at = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int64)).to(self._device)
            _, h, gain = self.pick_events(W, at, R)
            return h.cpu().numpy(), gain.cpu().numpy()

        def refit(sample, plane, shift, strength, n):
            if solve is not None:
                return self.solve_events(V, W, sample, plane, shift, strength, solve[0], solve[1])[0].cpu().numpy()
            return self.refit_events(V, W, sample, plane, shift, strength, n, 0., eps).cpu().numpy()
        return pursuit_loop(shape, self.atom_shape, self._sample_shape, self._reconstruction_mode, min_gain, max_events,
                            max_rounds, refit_iterations if solve is None else 1, sample.cpu().numpy(), plane.cpu().numpy(),
                            shift.cpu().numpy().reshape(-1, k), strength.cpu().numpy(), candidates, score, refit)

    # -- events: the dictionary learnt from the detections ------------------------------------------------------------------
    def event_plane_list(self, plane: torch.Tensor, n_planes: int):
        """The plane list tnmf_hip_events_grad_W takes, built on the device for checked events: (by_plane [K] int32, the
        rows in a stable order of ascending plane; plane_start [n_planes + 1] int32; workspace, the float64 slabs of the
        segments)."""
        with self._timed('event_plane_list'):
            K = plane.numel()
            sorted_plane, by_plane = torch.sort(plane, stable=True)
            plane_start = torch.searchsorted(sorted_plane, torch.arange(n_planes + 1, dtype=torch.int64,
                                                                        device=self._device)).to(torch.int32).contiguous()
            taps = self.n_channels * int(np.prod(self.atom_shape))
            workspace = torch.empty((K // _lib.EVENT_SEGMENT + n_planes) * 2 * taps, dtype=torch.float64,
                                    device=self._device)
        return by_plane.to(torch.int32).contiguous(), plane_start, workspace

    def gradient_W_event_list(self, W: torch.Tensor, events: torch.Tensor, lists, strength: torch.Tensor,
                              R: torch.Tensor) -> torch.Tensor:
        """This rank's [neg | pos] of the W gradient of the events, [2, P, C, *A] for the dictionary ``W[P, C, *A]`` the
        planes index, R being the render of the same strengths; NOT yet summed over ranks -> tnmf_hip_events_grad_W."""
        self._check_W(W)
        by_plane, plane_start, workspace = lists
        assert strength.is_contiguous() and strength.dtype == self._torch_dtype and events.shape[0] == strength.numel()
        assert by_plane.numel() == strength.numel() and plane_start.numel() == W.shape[0] + 1
        assert R.is_contiguous() and R.dtype == self._torch_dtype and tuple(R.shape) == tuple(self._V_dev.shape)
        negpos = torch.empty((2,) + tuple(W.shape), dtype=W.dtype, device=W.device)
        self._events_call('events_grad_W', W, _ptr(events), _ptr(by_plane), _ptr(plane_start), _ptr(strength),
                          strength.numel(), _ptr(self._V_dev), _ptr(R), _ptr(workspace), _ptr(negpos))
        return negpos

    def update_W_event_list(self, W: torch.Tensor, W_eff: Optional[torch.Tensor], transforms, negpos_eff: torch.Tensor,
                            eps: float = 1e-9) -> None:
        """The tail of the dense W half step on the gradient of the events, in place on W (and W_eff): fold, all-reduce,
        MU + normalise, expand.  An atom without evidence -- its summed neg, folded and all-reduced, is exactly zero in
        every entry: no events, only zero strengths, or only zero data under them -- keeps its entries, where the dense
        step would make it 0 / 0; the rule is a select on the device from the all-reduced buffer, the same on every rank."""
        negpos = negpos_eff if transforms is None else self.fold_gradient_W(negpos_eff, transforms)
        self._all_reduce(negpos)
        keep = ~negpos[0].reshape(W.shape[0], -1).any(dim=1)
        kept = W.clone()
        if transforms is None:
            self.apply_W(W, negpos, eps)
        elif self._world == 1:
            self.apply_W_transformed(W, W_eff, negpos_eff, transforms, eps)   # (the same bits as apply_W + expand_W)
        else:
            self.apply_W(W, negpos, eps)
        W.copy_(torch.where(keep.reshape((-1,) + (1,) * (W.dim() - 1)), kept, W))
        if transforms is not None:
            self.expand_W(W, transforms, W_eff)

    def fit_events(self, V, W: torch.Tensor, W_eff: Optional[torch.Tensor], transforms, sample, plane, shift, strength,
                   n_iterations: int, update_H: bool = True, update_W: bool = True, sparsity: float = 0.,
                   eps: float = 1e-9) -> torch.Tensor:
        """[K] strengths after ``n_iterations`` alternating multiplicative updates on the fixed support: of the strengths
        (update_H: the step of refit_events) and of the dictionary (update_W: the dense W half step on activations that are
        zero off the support), W and W_eff updated in place (W_eff is None without transforms).  The plain Frobenius
        objective.  With a process group the calls are collective: every rank calls with its own events (possibly none) and
        the same ``n_iterations``."""
        D = W if transforms is None else W_eff
        images, cell_start, events, strength, _ = self._prepared_events('fit_events', D.shape[0], sample, plane, shift,
                                                                        strength)
        # (column 1 of the rows: the checked planes)
        lists = self.event_plane_list(events[:, 1].to(torch.int64), D.shape[0]) if update_W else None
        strength = strength.clone()
        R = torch.empty_like(self._V_dev)
        for _ in range(int(n_iterations)):
            if update_H:
                self.render_event_list(D, images, cell_start, strength, R)
                self.update_event_list(D, events, strength, R, sparsity, eps)
            if update_W:
                self.render_event_list(D, images, cell_start, strength, R)
                negpos_eff = self.gradient_W_event_list(D, events, lists, strength, R)
                self.update_W_event_list(W, W_eff, transforms, negpos_eff, eps)
        return strength

    # -- a whole mini-batch epoch in one call -------------------------------------------------------------------
    @property
    def supports_schedules(self) -> bool:
        """tnmf_hip_run_schedule covers 'valid' mode on one device (with several ranks the W gradient must cross the
        collective between two of its operations)."""
        return self._mode == 0 and self._world == 1

    def prefers_schedule(self, H: torch.Tensor) -> bool:
        """A whole problem this small is bound by launch latency (BASELINE config 1: 0.34 ms per iteration for 0.1 ms of
        kernels): its full-batch iterations go through run_schedule, i.e. the persistent schedule kernel."""
        return self.supports_schedules and H.shape[0] > 0 and H.numel() <= (1 << 18)

    def blend_gradient_W(self, acc: torch.Tensor, g: torch.Tensor, a: float, b: float) -> torch.Tensor:
        """acc = a * acc + b * g in place (a == 0: acc = b * g) -- the accumulators of the mini-batch schedules
        (reference: TransformInvariantNMF.py:444-455) as a library kernel (tnmf_hip_axpby)."""
        assert acc.is_contiguous() and g.is_contiguous() and acc.shape == g.shape and acc.dtype == g.dtype
        _lib.check(self._lib.tnmf_hip_axpby(self._ctx, self._dtype_code, _ptr(acc), _ptr(g), float(a), float(b),
                                            acc.numel(), self._stream()), 'tnmf_hip_axpby')
        return acc

    def new_gradient_accumulator(self, W: torch.Tensor) -> torch.Tensor:
        return torch.empty((2,) + tuple(W.shape), dtype=W.dtype, device=W.device)

    def run_schedule(self, V, W: torch.Tensor, H: torch.Tensor, ops, acc: torch.Tensor, sparsity: float = 0.,
                     eps: float = 1e-9) -> None:
        """ops: sequence of ('H', slice) | ('G', slice, a, b) | ('W',) -- H half step on the slice, acc = a * acc +
        b * gradient_W(slice), W update from acc (reference: TransformInvariantNMF.py:444-504) -- issued by ONE call of
        the library (tnmf_hip_run_schedule): no interpreter time and no host round trip between the batch steps."""
        assert self.supports_schedules
        if self._G_dev is not None:
            raise NotImplementedError('run_schedule is unweighted; a weighted fit runs its epochs step by step')
        self._check_W(W)
        self._check_H(H, W.shape[0])
        ld = self._row_stride(H)
        assert ld is not None and H.shape[0] == self.n_local_samples
        assert acc.is_contiguous() and tuple(acc.shape) == (2,) + tuple(W.shape)
        assert acc.dtype == W.dtype and acc.device == W.device   # (the library writes 2 * |W| elements of W's type)
        arr = (_lib.Op * max(1, len(ops)))()
        for i, op in enumerate(ops):
            if op[0] == 'W':
                arr[i].kind, arr[i].n0, arr[i].n1 = _lib.OP_APPLY_W, 0, 0
                continue
            sl = self._local(op[1])
            arr[i].n0, arr[i].n1 = sl.start, sl.stop
            if op[0] == 'H':
                arr[i].kind = _lib.OP_UPDATE_H
            else:
                arr[i].kind, arr[i].a, arr[i].b = _lib.OP_GRAD_W, float(op[2]), float(op[3])

        def run(Hc, ld):
            with self._timed('schedule'):
                return self._lib.tnmf_hip_run_schedule(
                    self._ctx, ctypes.byref(self._geom(Hc.shape[0], W.shape[0], ld)), _ptr(self._V_dev), _ptr(W),
                    _ptr(Hc), _ptr(self._R_scratch), _ptr(acc), arr, len(ops), float(eps), float(sparsity),
                    self._stream()), 'tnmf_hip_run_schedule'
        self._call_resident_H(H, W, True, run)

    def apply_W(self, W: torch.Tensor, negpos: torch.Tensor, eps: float = 1e-9) -> None:
        """W = W * neg / (pos + eps), then normalise over the atom axes (TransformInvariantNMF.py:232-238)."""
        self._check_W(W)
        assert negpos.is_contiguous() and tuple(negpos.shape) == (2,) + tuple(W.shape)
        assert negpos.dtype == W.dtype and negpos.device == W.device
        g = self._geom(0, W.shape[0])
        with self._timed('apply_W'):
            _lib.check(self._lib.tnmf_hip_apply_W(self._ctx, ctypes.byref(g), _ptr(W), _ptr(negpos), float(eps),
                                                  self._stream()), 'tnmf_hip_apply_W')

    def local_gradient_W(self, V, W: torch.Tensor, H: torch.Tensor, s: slice = sliceNone, beta: float = 2.,
                         eps: float = 1e-9) -> torch.Tensor:
        """This rank's [neg | pos] of the W gradient as one [2, M, C, *A] buffer, NOT yet summed over ranks
        -> tnmf_hip_grad_W_beta (beta == 2: tnmf_hip_grad_W_fused); with weights bound tnmf_hip_grad_W_weighted."""
        self._check_beta(beta)
        ls = self._local(s)
        Hs, Vs = H[ls], self._V_dev[ls]
        self._check_W(W)
        self._check_H(Hs, W.shape[0])
        Hs = self._pad(Hs)
        negpos = torch.empty_like(self._negpos)
        Rs = self._R_scratch[ls] if Hs.shape[0] else None
        Gs = self._G(ls)

        def run(Hc, ld):
            g = self._geom(Hc.shape[0], W.shape[0], ld)
            r_valid = 0
            if self._timeline is not None and Hc.shape[0]:
                with self._timed('reconstruct'):
                    rc = self._lib.tnmf_hip_reconstruct(self._ctx, ctypes.byref(g), _ptr(W), _ptr(Hc), _ptr(Rs),
                                                        self._stream())
                if rc != 0:
                    return rc, 'tnmf_hip_reconstruct'
                r_valid = 1
            with self._timed('grad_W'):
                if Gs is not None:
                    return self._lib.tnmf_hip_grad_W_weighted(
                        self._ctx, ctypes.byref(g), _ptr(Vs), Gs, _ptr(W), _ptr(Hc), _ptr(Rs), r_valid, _ptr(negpos),
                        float(beta), float(eps), self._stream()), 'tnmf_hip_grad_W_weighted'
                rc = self._lib.tnmf_hip_grad_W_beta(self._ctx, ctypes.byref(g), _ptr(Vs), _ptr(W), _ptr(Hc), _ptr(Rs),
                                                    r_valid, _ptr(negpos), float(beta), float(eps), self._stream())
            return rc, 'tnmf_hip_grad_W_beta'
        self._call_resident_H(Hs, W, False, run)
        return negpos

    def all_reduce_gradient_W(self, negpos: torch.Tensor) -> torch.Tensor:
        """Sum a [neg | pos] buffer over the ranks of the process group (one RCCL all-reduce over xGMI)."""
        self._all_reduce(negpos)
        return negpos

    def fused_update_W(self, V, W: torch.Tensor, H: torch.Tensor, s: slice = sliceNone, eps: float = 1e-9,
                       beta: float = 2.) -> None:
        """One W half step, in place: local gradient, all-reduce over the ranks, MU + normalise
        (reference: TransformInvariantNMF.py:240-244)."""
        negpos = self.local_gradient_W(V, W, H, s, beta=beta, eps=eps)
        self._all_reduce(negpos)
        self.apply_W(W, negpos, eps)

    # -- transform groups and atom operators --------------------------------------------------------------------------
    # (transforms: a group name -> tnmf_hip_group_*, or an AtomOperators -> tnmf_hip_ops_* with this context's handle)
    def expand_W(self, W: torch.Tensor, transforms, W_eff: Optional[torch.Tensor] = None) -> torch.Tensor:
        """W_eff[m * T + t] = T_t(W[m]) -> tnmf_hip_group_expand_W / tnmf_hip_ops_expand_W (into W_eff when given; it drops
        the cached spectra of the dictionary)."""
        kind, arg = self._transform_arg(transforms)
        self._check_W(W)
        shape = (W.shape[0] * _transforms.size(transforms),) + tuple(W.shape[1:])
        if W_eff is None:
            W_eff = torch.empty(shape, dtype=W.dtype, device=W.device)
        self._check_W(W_eff)
        assert tuple(W_eff.shape) == shape
        g = self._geom(0, W.shape[0])
        name = f'tnmf_hip_{kind}_expand_W'
        with self._timed(f'{kind}_expand_W'):
            _lib.check(getattr(self._lib, name)(self._ctx, ctypes.byref(g), arg, _ptr(W), _ptr(W_eff), self._stream()),
                       name)
        return W_eff

    def fold_gradient_W(self, negpos_eff: torch.Tensor, transforms) -> torch.Tensor:
        """[neg | pos] of W_eff ([2, M * T, C, *A]) -> [neg | pos] of W ([2, M, C, *A]) -> tnmf_hip_group_fold_grad_W /
        tnmf_hip_ops_fold_grad_W."""
        kind, arg = self._transform_arg(transforms)
        T = _transforms.size(transforms)
        assert negpos_eff.is_contiguous() and negpos_eff.dtype == self._torch_dtype and negpos_eff.shape[1] % T == 0
        assert tuple(negpos_eff.shape[2:]) == (self.n_channels,) + self.atom_shape and negpos_eff.shape[0] == 2
        M = negpos_eff.shape[1] // T
        negpos = torch.empty((2, M) + tuple(negpos_eff.shape[2:]), dtype=negpos_eff.dtype, device=negpos_eff.device)
        g = self._geom(0, M)
        name = f'tnmf_hip_{kind}_fold_grad_W'
        with self._timed(f'{kind}_fold_grad_W'):
            _lib.check(getattr(self._lib, name)(self._ctx, ctypes.byref(g), arg, _ptr(negpos_eff), _ptr(negpos),
                                                self._stream()), name)
        return negpos

    def apply_W_transformed(self, W: torch.Tensor, W_eff: torch.Tensor, negpos_eff: torch.Tensor, transforms,
                            eps: float = 1e-9) -> None:
        """Fold, W = W * neg / (pos + eps), normalise, expand into W_eff: one launch (tnmf_hip_group_apply_W /
        tnmf_hip_ops_apply_W), the same bits as fold_gradient_W -> apply_W -> expand_W."""
        kind, arg = self._transform_arg(transforms)
        self._check_W(W)
        self._check_W(W_eff)
        T = _transforms.size(transforms)
        assert W_eff.shape[0] == W.shape[0] * T
        assert negpos_eff.is_contiguous() and tuple(negpos_eff.shape) == (2,) + tuple(W_eff.shape)
        assert negpos_eff.dtype == W.dtype and negpos_eff.device == W.device
        g = self._geom(0, W.shape[0])
        name = f'tnmf_hip_{kind}_apply_W'
        with self._timed(f'{kind}_apply_W'):
            _lib.check(getattr(self._lib, name)(self._ctx, ctypes.byref(g), arg, _ptr(W), _ptr(W_eff), _ptr(negpos_eff),
                                                float(eps), self._stream()), name)

    def fused_update_W_transformed(self, V, W: torch.Tensor, W_eff: torch.Tensor, H: torch.Tensor, s: slice = sliceNone,
                                   transforms=None, eps: float = 1e-9, beta: float = 2.) -> None:
        """One W half step of a transformed model, in place on W and W_eff: the local gradient of W_eff; on one rank the
        fused fold + MU + normalise + expand; on several the fold, the all-reduce of the M-atom buffer, apply_W and
        expand_W."""
        negpos_eff = self.local_gradient_W(V, W_eff, H, s, beta=beta, eps=eps)
        if self._world == 1:
            self.apply_W_transformed(W, W_eff, negpos_eff, transforms, eps)
            return
        negpos = self.fold_gradient_W(negpos_eff, transforms)
        self._all_reduce(negpos)
        self.apply_W(W, negpos, eps)
        self.expand_W(W, transforms, W_eff)
