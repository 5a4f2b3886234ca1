"""
CPU guard of the launch convention ("one launch per precision pair"): every launcher reaches its float and double
kernels through with_dtype() of common.h, written once as <T>, and the events family sizes its grids with events_grid() of
events.h.  Sources read as text; no GPU, no build.
"""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')
SOURCES = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')))
EVENTS_FILES = ('events.hip', 'solve.hip', 'pursuit.hip', 'landscape.hip', 'alternatives.hip')
# the one spelled-out pair: double transforms exist only up to L = 288, so the double arm sits under `if constexpr`
SPELLED_OUT = {'fft_len.hip': {'fft_run_typed'}}


def _read(path):
    with open(path) as f:
        return f.read()


def _flat(text):
    return re.sub(r'\s+', ' ', text)


def _used_with(text, T):
    """Every name used with <T...> spelled out: k_x<T>, (k_x<T, true>), launch_x<T>(...).  The declarator of an explicit
    specialisation (`template <> struct Vec<double> {`) is a definition, not a use."""
    return set(re.findall(r'(\w+)<%s\b' % T, re.sub(r'template\s*<>[^{;]*', '', text)))


def test_common_h_defines_the_helper_with_both_arms_and_the_element_size():
    common = _flat(_read(os.path.join(CSRC, 'common.h')))
    assert ('template <typename F> static inline decltype(auto) with_dtype(int dtype, F &&f) { '
            'if (dtype == 0) return f(float{}); return f(double{}); }') in common
    assert 'static inline size_t esize(int dtype) { return dtype == 0 ? 4 : 8; }' in common
    assert sum('size_t esize(' in _read(p) for p in SOURCES) == 1


def test_no_kernel_is_spelled_out_in_both_precisions():
    sources = [p for p in SOURCES if p.endswith('.hip')]
    assert len(sources) >= 19
    for path in sources:
        text, name = _read(path), os.path.basename(path)
        both = _used_with(text, 'float') & _used_with(text, 'double')
        assert both == SPELLED_OUT.get(name, set()), (name, both)
    # the matcher sees a twin where there is one
    twin = 'if (dtype == 0) hipLaunchKernelGGL(k_a<float>, g); else hipLaunchKernelGGL(k_a<double>, g);'
    assert _used_with(twin, 'float') & _used_with(twin, 'double') == {'k_a'}
    twin = 'return dtype == 0 ? launch_x<float>(a) : launch_x<double>(a); hipLaunchKernelGGL((k_b<float, true>), g)'
    assert _used_with(twin, 'float') == {'launch_x', 'k_b'} and _used_with(twin, 'double') == {'launch_x'}


def test_the_private_macros_and_helpers_are_gone():
    for path in SOURCES:
        text = _read(path)
        for word in ('LAUNCH_PF', 'VOL_CW', 'SPEC_R_T', 'SPEC_G_T', 'esz_of'):
            assert word not in text, (os.path.basename(path), word)
        if os.path.basename(path) != 'common.h':
            assert '? 4 : 8' not in text.replace('L > 288 ? 4 : 8', ''), os.path.basename(path)


def test_the_events_family_takes_frames_and_one_grid_rule():
    for name in EVENTS_FILES:
        assert 'grid_for' not in _read(os.path.join(CSRC, name)), name
    events_h = _flat(_read(os.path.join(CSRC, 'events.h')))
    assert 'struct EventFrame { EventGeo g; int mode, Sy, Sx; };' in events_h
    assert ('inline unsigned events_grid(const tnmf_hip_ctx *ctx, long long blocks, int per_cu = 64) { return (unsigned)'
            'std::max<long long>(1, std::min<long long>(blocks, (long long)ctx->num_cu * per_cu)); }') in events_h
    # every call site with its workgroups per CU; those of events.hip and solve.hip (the default, 64) are pinned by
    # test_events_dispatch_cpu.py and test_solve_dispatch_cpu.py
    sites = {'events.hip': 3, 'solve.hip': 3,
             'pursuit.hip': ['events_grid(ctx, cdiv(entries, kEventThreads), 8)',
                             'events_grid(ctx, (rows * cpr + kEventThreads - 1) / kEventThreads, 8)',
                             'events_grid(ctx, (n_taken + kEventThreads - 1) / kEventThreads, 8)',
                             'events_grid(ctx, (n_picked + kWaves - 1) / kWaves, 64)'],
             'landscape.hip': ['events_grid(ctx, (n_events + kWaves - 1) / kWaves, TNMF_LANDSCAPE_BLOCKS_PER_CU)'],
             'alternatives.hip': ['events_grid(ctx, (n_events + kWaves - 1) / kWaves, TNMF_ALTERNATIVES_BLOCKS_PER_CU)']}
    for name, calls in sites.items():
        flat = _flat(_read(os.path.join(CSRC, name)))
        assert flat.count('events_grid(') == (calls if isinstance(calls, int) else len(calls)), name
        assert isinstance(calls, int) or all(call in flat for call in calls), name
    # the nine launchers take the frame, and the kernels get its four parts in the order they always had
    decls = events_h + _flat(_read(os.path.join(CSRC, 'solve.h')))
    for fn in ('events_update', 'events_gain', 'events_grad_W', 'events_norms', 'pursuit_pick', 'events_landscape',
               'events_alternatives', 'events_gram', 'events_project'):
        assert f'int {fn}(tnmf_hip_ctx *ctx, const EventFrame &f, ' in decls, fn
    assert 'int mode, int Sy, int Sx' not in decls
    family = ''.join(_flat(_read(os.path.join(CSRC, n))) for n in EVENTS_FILES)
    assert family.count(', s, g, f.mode, f.Sy, f.Sx, ') + family.count(', s, f.g, f.mode, f.Sy, f.Sx, ') == 9
