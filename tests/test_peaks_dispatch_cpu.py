"""
CPU guard of the peaks kernel matrix: the host mirror of the launch of k_find_peaks (tests/peaks_dispatch.py) is held to
the source it restates, and the calls of tests/test_hip_peaks_matrix.py, with those of tests/test_hip_peaks.py, are held to
executing every named branch of the plain form, each item of the list the matrix was built for (P1-P7) through a call named
for it.  No GPU, no build: the sources are read as text.
"""
import os
import re

import numpy as np
import pytest

import peaks_dispatch as pd
import peaks_reference as pref
import test_hip_peaks as old
import test_hip_peaks_matrix as gm
from conftest import ROOT

CSRC = os.path.join(ROOT, 'tnmf_amd', 'csrc')


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


# the calls of tests/test_hip_peaks.py through check_case: (shape, row stride, thresholds, radius, group)
OLD_CALLS = [((3, 8, 19, 37), 64, (0., 2.), radius, group) for radius in ((3, 5), (0, 0), (40, 40)) for group in (1, 4, 8)]
OLD_CALLS += [((2, 3, 33, 32), None, (0., 2.), (2, 3), 1), ((2, 3, 33, 32), None, (0., 2.), (1, 40), 3),
              ((2, 3, 70, 130), None, (0., 2.), (11, 11), 1)]
OLD_CALLS += [((2, 5, 300), None, (0., 2.), (radius,), group) for radius in (0, 63) for group in (1, 5)]
OLD_CALLS += [((2, 4, 6, 7, 9), None, (0., 2.), (1, 2, 3), group) for group in (1, 2)]


def test_the_old_calls_are_those_of_the_old_file():
    src = _read('tests', 'test_hip_peaks.py')
    for line in ("@pytest.mark.parametrize('group', [1, 4, 8])",
                 "@pytest.mark.parametrize('radius', [(3, 5), (0, 0), (40, 40)], ids=str)",
                 'check_case(ctx, (3, 8, 19, 37), 1, dtype, 64, threshold, radius, group)',
                 'check_case(ctx, (2, 3, 33, 32), 2, dtype, None, threshold, (2, 3), 1)',
                 'check_case(ctx, (2, 3, 33, 32), 2, dtype, None, threshold, (1, 40), 3)',
                 'check_case(ctx, (2, 3, 70, 130), 3, dtype, None, threshold, (11, 11), 1)',
                 "@pytest.mark.parametrize('radius', [0, 63])",
                 'check_case(ctx, (2, 5, 300), 4, dtype, None, threshold, (radius,), 1)',
                 'check_case(ctx, (2, 5, 300), 4, dtype, None, threshold, (radius,), 5)',
                 'check_case(ctx, (2, 4, 6, 7, 9), 5, 0, None, threshold, (1, 2, 3), group)'):
        assert line in src, line
    assert src.count("@pytest.mark.parametrize('threshold', [0., 2.])") == 5


# -- the mirror against the source ----------------------------------------------------------------------------------------------
def test_constants_are_those_of_the_source():
    src = _read(CSRC, 'peaks.hip')
    assert pd.WAVES == int(re.search(r'constexpr int kWaves = (\d+);', src).group(1))
    assert pd.ROWS_PER_WAVE == int(re.search(r'constexpr int kRowsPerWave = (\d+);', src).group(1))
    assert pd.SLAB_BATCH == int(re.search(r'constexpr int kSlabBatch = (\d+);', src).group(1))
    assert 'constexpr int kBlockRows = kWaves * kRowsPerWave;' in src and pd.BLOCK_ROWS == pd.WAVES * pd.ROWS_PER_WAVE
    m = re.search(r'const unsigned gx = \(unsigned\)std::min\(\(rpp \+ kBlockRows - 1\) / kBlockRows, (\d+)\);', src)
    assert m and pd.GX_CAP == int(m.group(1))
    assert f'std::min<long long>(g.planes, budget), {pd.GY_CAP}));' in src


def test_mirrored_rules_are_those_of_the_source():
    """The lines the mirror restates.  When one of them changes, tests/peaks_dispatch.py and the calls of the matrix have to
    be looked at again."""
    src = _read(CSRC, 'peaks.hip')
    for line in ('const int width = std::min(2 * g_in.rx + 1, g_in.Sx);',
                 'while (w.lw < 6 && (1 << w.lw) < width) ++w.lw;',
                 'const int wpad = 1 << w.lw, rpi = 64 >> w.lw;',
                 'const bool tiled = false && tile_bytes <= kMaxTileBytes;',
                 'if (g.Sz == 1 && g.Sy == 1 && g.group == 1 && g.planes <= 0x7fffffffLL) {',
                 'const int rpp = g.Sz * g.Sy;',
                 'const long long budget = std::max<long long>(1, (long long)ctx->num_cu * 64 / gx);',
                 'for (long long plane = blockIdx.y; plane < g.planes; plane += gridDim.y) {',
                 'if (g.group > 1) qc = (int)(plane % g.P) % g.group;',
                 'for (int rb = blockIdx.x * kBlockRows; rb < rpp; rb += gridDim.x * kBlockRows) {',
                 'for (int xb = 0; xb < g.Sx; xb += 64) {',
                 'if (g.rx >= 1) {',
                 'if (g.ry >= 1 && g.Sz == 1) {   // (one plane of two axes: the wave\'s rows are neighbours in y)',
                 'for (int xs = x0; xs <= x1 && !suppressed; xs += wpad) {',
                 'for (int j0 = 0; j0 < n_rows; j0 += kSlabBatch * rpi) {',
                 'if ((double)f > t) f = nextafterf(f, -INFINITY);'):
        assert line in src, line
    api = _read(CSRC, 'api.hip')
    assert 'r[k] = std::min(radius[i], S[k] - 1);   // (a radius at or beyond the extent: the whole axis)' in api
    assert 'NaN compares false: never a detection, never a suppressor' in ' '.join(_read('include', 'tnmf_hip.h').split()) \
        .replace(' * ', ' ')


def test_launches_of_the_matrix():
    """The figures the comments of the matrix quote, on 256 compute units."""
    def c(name):
        shape, _, stride, _, radius, group = pd.call_of(name)
        return pd.launch(shape, radius, group, stride)
    ps = c('plane-stride')
    assert (ps.planes, ps.gx, ps.gy, ps.plane_loop_strides, ps.fold) == (16560, 1, 16384, True, False)
    assert not c('plane-stride-group-4').qc_changes and c('plane-stride-group-3').qc_changes
    rs = c('row-stride')
    assert (rs.fold, rs.rpp, rs.gx, rs.gy, rs.row_loop_strides, rs.plane_loop_strides) == (True, 16896, 1024, 1, True, False)
    v, h = c('vertical-only'), c('horizontal-only')
    assert (v.lw, v.rpi, v.thin_x, v.thin_y, v.n_rows) == (0, 64, False, True, 9)
    assert (h.lw, h.rpi, h.thin_x, h.thin_y, h.n_rows) == (4, 4, True, False, 1)
    assert (c('narrow-3').width, c('narrow-3').lw, c('narrow-2').width, c('narrow-2').lw) == (3, 2, 2, 1)
    w = c('wide-2d')
    assert (w.width, w.lw, w.rpi, w.xs_steps, w.n_rows, w.j0_batches) == (81, 6, 1, 2, 3, 1)


@pytest.mark.parametrize('num_cu', [64, 256, 304])
def test_the_plane_stride_calls_stride_on_any_cu_count(num_cu):
    for name in ('plane-stride', 'plane-stride-group-4', 'plane-stride-group-3'):
        shape, _, stride, _, radius, group = pd.call_of(name, num_cu)
        c = pd.launch(shape, radius, group, stride, num_cu)
        assert c.plane_loop_strides and c.planes - c.gy < 240, (name, c)   # (the fewest samples that do)
    assert pd.launch(pd.call_of('row-stride', num_cu)[0], (2,), 1, None, num_cu).row_loop_strides


# -- the matrix against the mirror ----------------------------------------------------------------------------------------------
def _all_calls():
    """name -> the sets of branches its calls reach (both element types)."""
    out = {}
    for name in pd.MATRIX:
        shape, _, stride, threshold, radius, group = pd.call_of(name)
        out[name] = set().union(*[pd.reached(shape, radius, group, stride, threshold, dt) for dt in (0, 1)])
    out['threshold-ulp'] = set().union(*[pd.reached(pd.ULP_SHAPE, (0, 0), 1, stride, pd.ULP_THRESHOLD, dt)
                                         for dt in (0, 1) for stride in (None, 128)])
    out['nan-inf'] = set().union(*[pd.reached(pd.NAN_INF_SHAPE, radius, group, None, t, dt)
                                   for radius, group in pd.NAN_INF_CALLS for t in (0., 2.) for dt in (0, 1)])
    for i, (shape, stride, thresholds, radius, group) in enumerate(OLD_CALLS):
        out[f'old:{i}'] = set().union(*[pd.reached(shape, radius, group, stride, t, dt) for t in thresholds for dt in (0, 1)])
    return out


def test_the_calls_together_reach_every_branch():
    union = set().union(*_all_calls().values())
    assert union == set(pd.BRANCHES), sorted(set(pd.BRANCHES) - union)


def test_every_new_item_is_reached_by_a_call_named_for_it():
    """Each name that stands for P1-P6 is claimed by a call of the matrix that reaches it, and no call of the old file
    reached it; P7 is a property of the input, checked below."""
    calls = _all_calls()
    claimed = {}
    for name, entry in pd.MATRIX.items():
        assert entry[6], name
        for b in entry[6]:
            assert b in pd.NEW, (name, b)
            assert b in calls[name], f'{name} no longer reaches {b}'
            claimed.setdefault(b, []).append(name)
    assert 'P6:threshold-rounded-down' in calls['threshold-ulp']
    claimed['P6:threshold-rounded-down'] = ['threshold-ulp']
    for b in pd.NEW:
        assert claimed.get(b), f'no call of the matrix is named for {b}'
    assert {b[:2] for b in pd.NEW} == {f'P{i}' for i in range(1, 7)}
    before = set().union(*[names for name, names in calls.items() if name.startswith('old:')])
    assert not before & set(pd.NEW), sorted(before & set(pd.NEW))


# -- the inputs: neither nothing nor everything is detected -------------------------------------------------------------------
@pytest.mark.parametrize('name', list(pd.MATRIX))
def test_the_reference_detects_something_and_not_everything(name):
    shape, seed, _, threshold, radius, group = pd.call_of(name)
    want = old.reference(shape, seed, threshold, radius, group)      # (asserts 0 < detections < entries)
    assert 0 < len(want) < int(np.prod(shape))


def test_the_threshold_input_decides_on_one_ulp():
    """P6: the entries one float32 step apart fall on both sides of the threshold, in both element types."""
    t32 = np.float32(pd.ULP_THRESHOLD)
    assert pd.threshold_rounds_down(pd.ULP_THRESHOLD, 0) and not pd.threshold_rounds_down(pd.ULP_THRESHOLD, 1)
    assert not pd.threshold_rounds_down(0., 0) and not pd.threshold_rounds_down(2., 0)
    for dtype in (0, 1):
        H, want = gm.ulp_input(dtype)
        flat = H.reshape(-1)
        assert np.array_equal(flat.astype(gm.NP_DTYPES[dtype]).astype(np.float64), flat)   # exact in the element type
        detected = np.zeros(H.size, dtype=bool)
        detected[want] = True
        assert detected[flat == float(t32)].all() and not detected[flat == float(np.nextafter(t32, np.float32(0)))].any()
        assert not detected[flat == pd.ULP_THRESHOLD].any() and (dtype == 0 or np.any(flat == pd.ULP_THRESHOLD))


def test_the_nan_inf_input_holds_what_it_is_for():
    """P7: NaN and +inf lie inside the windows of detections, +inf is detected, and two +inf compete."""
    H = gm.nan_inf_input()
    assert np.isnan(H).any() and np.isinf(H).any() and not np.isneginf(H).any()
    for radius, group in pd.NAN_INF_CALLS:
        want = gm.nan_inf_reference(radius, group, 0.)
        vals = H.reshape(-1)[want]
        assert not np.isnan(vals).any()
        # NaN is no suppressor: with every NaN replaced by 0 (an entry that suppresses nothing above a threshold >= 0) the
        # reference's detections are the same
        same, _ = pref.find_peaks(np.where(np.isnan(H), 0., H), 0., radius, group)
        np.testing.assert_array_equal(same, want)
        if radius != (0, 0):
            assert 0 < np.isinf(vals).sum() < np.isinf(H).sum()     # some +inf suppressed by another: the tie by index
            at = np.stack(np.unravel_index(want, H.shape), axis=1)
            beside_nan = 0
            for n, q, y, x in at[:400]:
                box = H[n, q, max(y - radius[0], 0):y + radius[0] + 1, max(x - radius[1], 0):x + radius[1] + 1]
                beside_nan += bool(np.isnan(box).any())
            assert beside_nan > 5
