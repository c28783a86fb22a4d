"""The five kernels of trm_field_io_api.hip -- k_transpose, k_rows_to_host_layout, k_scatter_ring, k_gather_ring, k_reduce_rows -- at
the shapes where they take another path: Nh and Nz next to the 32 x 32 tile, Nz past one tile row (Nzp = 32, 64, then multiples of
32), partial waves and blocks of the reduction, and Nh = 65 536 + 257 where its grid-stride loop runs a second trip.

Values encode their position (host[k, i] = k * 4096 + i, integers below 2^24: exact in fp32 as well), so a wrong index cannot hide,
and every upload is read back by paths that do not share its kernel: the z-fastest device buffer itself (device_array, padding
levels included), the row reader, the ring scatter and the reductions, whose results have closed forms.  Reductions of random data
are held to math.fsum with the a-priori bounds of recursive summation in double, and to Julia's Base.minimum / maximum on NaN,
infinities and zeros of both signs.  The per-case error-to-bound ratios are printed (pytest -s); the largest are in DESIGN.md 4.3.
"""
import functools
import math

import numpy as np
import pytest

import terrarium_jl_amd as trm
import ring_oracle as R

pytestmark = pytest.mark.gpu

EINVAL, ESTALE = trm._capi.TRM_EINVAL, trm._capi.TRM_ESTALE
U = 2.0 ** -53                                  # unit roundoff of double
OPS = ("sum", "min", "max", "hasnan", "volume_integral_z")

# (Nh, Nz): every Nh of {1, 31, 32, 33, 63, 65, 255, 257} and every Nz of {2, 31, 32, 33, 64, 65, 97} at least once; Nz = 97 gives
# Nzp = 128, four tile rows, the last one partly padding.  (trm_create refuses Nz = 1: test_one_layer_grids_do_not_exist.)
PAIRS = [(1, 2), (33, 33), (257, 65), (31, 97), (32, 31), (32, 32), (63, 32), (65, 64), (255, 33), (255, 2), (33, 31), (1, 65)]
DTYPES = [np.float64, np.float32]
SHAPES = [(Nh, Nz, dt) for Nh, Nz in PAIRS for dt in DTYPES]
LARGE = (65536 + 257, 2, np.float32)            # reductions only: the second trip of the stride loop holds one full and one partial block


def shape_id(s):
    return f"Nh{s[0]}-Nz{s[1]}-{np.dtype(s[2]).name}"


def fresh_state(Nh, Nz, dtype, **kw):
    grid = trm.ColumnGrid(trm.ExponentialSpacing(N=Nz), num_columns=Nh, dtype=dtype)
    return trm.initialize(trm.SoilModel(grid), trm.ForwardEuler(dt=60.0), **kw).state


@functools.lru_cache(maxsize=None)
def _shared_state(Nh, Nz, dtype_name):
    return fresh_state(Nh, Nz, np.dtype(dtype_name))


def state_of(shape):
    """One context per shape for the tests that never step: each of them uploads what it reads."""
    Nh, Nz, dtype = shape
    return _shared_state(Nh, Nz, np.dtype(dtype).name)


def nzp_of(Nz):
    return 32 if Nz <= 32 else 64 if Nz <= 64 else (Nz + 31) // 32 * 32


def encoded(rows, Nh, dtype):
    return (np.arange(rows)[:, None] * 4096 + np.arange(Nh)[None, :]).astype(dtype)


def encoded_large(rows, Nh, dtype):
    """(k - 1) * 2^22 + i: exact in fp32 and distinct over [3][2^17], both signs"""
    return ((np.arange(rows)[:, None] - 1) * 2 ** 22 + np.arange(Nh)[None, :]).astype(dtype)


def device_view(d, name):
    import torch
    return torch.as_tensor(d.device_array(name), device=f"cuda:{int(d.grid.device)}")


def view_to_host(d, name):
    import torch
    torch.cuda.synchronize()
    return device_view(d, name).cpu().numpy()


def torch_dtype(dtype):
    import torch
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def windows(rows):
    """(row0, nrows): the first row, the last row, everything, the last two, and windows around row 32 where the field has one"""
    w = [(0, 1), (rows - 1, 1), (0, rows), (max(0, rows - 2), min(2, rows))]
    if rows > 33:
        w += [(30, 5), (31, 2), (32, 1), (1, rows - 1)]
    if rows > 65:
        w += [(62, 5), (29, rows - 29)]
    return [(row0, min(nrows, rows - row0)) for row0, nrows in w]


def alternating_mask(Nh):
    mask = np.zeros(2 * Nh + 2, dtype=bool)
    mask[1 + 2 * np.arange(Nh)] = True
    return mask


def raises(code, match, call):
    with pytest.raises(trm.TerrariumHipError, match=match) as e:
        call()
    assert e.value.code == code, e.value
    return e


# ---- 1. transposition, read by paths that do not share its kernel --------------------------------------------------------------
def check_closed_form_reductions(d, name, rows, Nh, base):
    """rows of base(k) + i, i < Nh: min, max and sum are exact in double"""
    k = np.arange(rows, dtype=np.float64)
    assert np.array_equal(d.reduce(name, "min"), base(k)), name
    assert np.array_equal(d.reduce(name, "max"), base(k) + (Nh - 1)), name
    assert np.array_equal(d.reduce(name, "sum"), Nh * base(k) + Nh * (Nh - 1) / 2), name
    assert np.array_equal(d.reduce(name, "hasnan"), np.zeros(rows)), name


def other_pattern(Nz, Nh, dtype):
    """differs from encoded() in every element (halves are exact)"""
    return encoded(Nz, Nh, dtype)[::-1] + dtype(0.5)


def scrub(d):
    """Uploads and downloads pass the same staging buffers in the same layout: a download that wrote nothing at all would still hand
    back what the upload had staged.  Before a read under test both staging buffers (rows, ring) are made to hold another pattern."""
    d.get_ring("internal_energy", fill=-5.0)


def check_device_buffer(d, name, host, Nz):
    """the device buffer itself: level fastest, pitch Nzp, the padding levels zero; the top face of a Face field is not part of it"""
    dev = view_to_host(d, name)
    assert dev.shape == (host.shape[1], nzp_of(Nz)) and dev.dtype == host.dtype
    assert np.array_equal(dev[:, :Nz].T, host[:Nz]), name
    assert not dev[:, Nz:].any(), name


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_upload_is_read_back_exactly_five_ways(shape):
    Nh, Nz, dtype = shape
    d = state_of(shape)
    mask = alternating_mask(Nh)
    d.set_ring_grid(mask.size, np.flatnonzero(mask))
    other = other_pattern(Nz, Nh, dtype)
    d.set("internal_energy", other)
    check_device_buffer(d, "internal_energy", other, Nz)
    for name, rows in (("temperature", Nz), ("hydraulic_conductivity", Nz + 1)):
        host = encoded(rows, Nh, dtype)
        d.set(name, host)
        on_ring = R.ring_field_from_columns(host, mask)
        check_device_buffer(d, name, host, Nz)
        scrub(d)
        assert np.array_equal(d.get(name), host), name
        for row0, nrows in windows(rows):
            scrub(d)
            assert np.array_equal(d.get_rows(name, row0, nrows), host[row0:row0 + nrows]), (name, row0, nrows)
            scrub(d)
            assert np.array_equal(np.atleast_2d(d.get_ring(name, row0=row0, nrows=nrows)), on_ring[row0:row0 + nrows], equal_nan=True), (name, row0, nrows)
        check_closed_form_reductions(d, name, rows, Nh, lambda k: k * 4096.0)
    scrub(d)
    assert np.array_equal(d.get("ground_temperature"), encoded(Nz, Nh, dtype)[-1])
    d.get_ring("temperature", fill=-5.0)                # (the staging buffers hold the first pattern: the download of the other one)
    assert np.array_equal(d.get("internal_energy"), other)
    wt = (5 * 4096 + np.arange(Nh)).astype(dtype)
    d.set("water_table", wt)
    assert np.array_equal(view_to_host(d, "water_table"), wt)
    scrub(d)
    assert np.array_equal(d.get("water_table"), wt)
    scrub(d)
    assert np.array_equal(d.get_rows("water_table", 0, 1)[0], wt)
    scrub(d)
    assert np.array_equal(d.get_ring("water_table", fill=-3.0), R.ring_field_from_columns(wt, mask, -3.0))
    check_closed_form_reductions(d, "water_table", 1, Nh, lambda k: k + 5 * 4096.0)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_every_upload_path_zeroes_the_padding_levels(shape):
    """Levels Nz .. Nzp - 1 of a 3-D buffer are 0 after trm_upload, trm_upload_ring and trm_gather_ring_device, whatever they held:
    the buffer is filled with a pattern through its device view first, and read through that view afterwards."""
    import torch
    Nh, Nz, dtype = shape
    d = state_of(shape)
    mask = alternating_mask(Nh)
    d.set_ring_grid(mask.size, np.flatnonzero(mask))
    for name, rows in (("temperature", Nz), ("hydraulic_conductivity", Nz + 1)):
        host = encoded(rows, Nh, dtype)
        full = R.ring_field_from_columns(host, mask, -7.0)
        on_device = torch.as_tensor(full, device=f"cuda:{int(d.grid.device)}")
        torch.cuda.synchronize()
        for how in ("upload", "upload_ring", "gather_ring_device"):
            device_view(d, name).fill_(-12345.0)
            torch.cuda.synchronize()
            assert (view_to_host(d, name) == -12345.0).all()
            if how == "upload":
                d.set(name, host)
            elif how == "upload_ring":
                d.set_ring(name, full)
            else:
                d.gather_ring_from(name, on_device.data_ptr())
            dev = view_to_host(d, name)
            assert np.array_equal(dev[:, :Nz].T, host[:Nz]), (name, how)
            assert not dev[:, Nz:].any(), (name, how)
            assert np.array_equal(d.get(name), host), (name, how)


@pytest.mark.parametrize("Nh,Nz", [(33, 33), (31, 97)])
def test_a_step_does_not_see_what_the_padding_held(Nh, Nz):
    """One finalizing step of the heat-only model, bit for bit against a twin whose buffers never held the pattern."""
    import torch
    names = ("internal_energy", "temperature", "liquid_water_fraction", "saturation_water_ice")
    rng = np.random.default_rng([81, Nh, Nz])
    kw = dict(initializers=dict(temperature=rng.uniform(-4.0, 6.0, (Nz, Nh)), saturation_water_ice=rng.uniform(0.2, 0.9, (Nz, Nh))),
              boundary_conditions=trm.PrescribedSurfaceTemperature("T_ub", 3.0))
    a, b = fresh_state(Nh, Nz, np.float64, **kw), fresh_state(Nh, Nz, np.float64, **kw)
    for name in names:
        values = b.get(name)
        assert np.array_equal(a.get(name), values)
        device_view(a, name).fill_(1.0e30)
        device_view(b, name)                            # (handed out as well, never written: the same flags in both contexts)
        torch.cuda.synchronize()
        a.set(name, values)
        b.set(name, values)
    for d in (a, b):
        d.step(60.0, 1, finalize=True)
    for name in names + ("tend_internal_energy",):
        x, y = a.get(name), b.get(name)
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), name
    assert not np.array_equal(a.get("temperature"), kw["initializers"]["temperature"])
    assert a.status() == b.status() == 0


# ---- 2. ring scatter / gather at edges --------------------------------------------------------------------------------------------
def _ring_cases():
    seam = np.array(sorted(set(range(0, 900, 3)) | {255, 256, 257}))      # 302 columns: points and columns both cross 256
    return {
        "all_land": (33, np.arange(33), 33),                              # Nh = P: no fill at all
        "first_point": (300, np.array([0]), 2),
        "last_point": (300, np.array([299]), 2),
        "points_255_256_257": (600, np.array([3, 255, 256, 257, 511, 512, 599]), 33),
        "alternating_257": (257, np.arange(0, 257, 2), 2),
        "columns_across_256": (900, seam, 2),
    }


RING_CASES = _ring_cases()


def check_gathered(d, name, expect, Nz):
    """what a gather left in the field: in the device buffer itself, and through a download that starts from other staging contents"""
    if expect.shape[0] > 1:
        check_device_buffer(d, name, expect, Nz)
    else:
        assert np.array_equal(view_to_host(d, name), expect[0]), name
    scrub(d)
    assert np.array_equal(np.atleast_2d(d.get(name)), expect), name


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("case", sorted(RING_CASES))
def test_ring_scatter_and_gather_at_edges(case, dtype):
    import torch
    P, index, Nz = RING_CASES[case]
    Nh = index.size
    mask = np.zeros(P, dtype=bool)
    mask[index] = True
    d = state_of((Nh, Nz, dtype))
    d.set_ring_grid(P, index)
    dev = f"cuda:{int(d.grid.device)}"
    fill = 0.1                                                             # (not a float: the fp32 field must hold float32(0.1))
    d.set("internal_energy", other_pattern(Nz, Nh, dtype))                 # (what scrub() leaves in the staging buffers)
    for name, rows in (("temperature", Nz), ("hydraulic_conductivity", Nz + 1), ("water_table", 1)):
        host = encoded(rows, Nh, dtype)
        d.set(name, host if rows > 1 else host[0])
        # scatter to the host: NaN and a finite fill
        scrub(d)
        got = np.atleast_2d(d.get_ring(name))
        assert got.shape == (rows, P) and got.dtype == np.dtype(dtype)
        assert np.array_equal(got, R.ring_field_from_columns(host, mask), equal_nan=True), name
        scrub(d)
        got = np.atleast_2d(d.get_ring(name, fill=fill))
        filled, minus = R.ring_field_from_columns(host, mask, fill), R.ring_field_from_columns(host, mask, -1.0)
        assert np.array_equal(got, filled), name
        assert (got[:, ~mask] == dtype(fill)).all() and np.isnan(np.atleast_2d(d.get_ring(name))[:, ~mask]).all()
        for row0, nrows in windows(rows):
            scrub(d)
            assert np.array_equal(np.atleast_2d(d.get_ring(name, fill=fill, row0=row0, nrows=nrows)), filled[row0:row0 + nrows]), (name, row0, nrows)
            buf = torch.full((nrows, P), 77.0, dtype=torch_dtype(dtype), device=dev)
            torch.cuda.synchronize()
            scrub(d)
            d.scatter_ring_to(name, buf.data_ptr(), fill=-1.0, row0=row0, nrows=nrows)
            torch.cuda.synchronize()
            assert np.array_equal(buf.cpu().numpy(), minus[row0:row0 + nrows]), (name, row0, nrows)
        # gather: from the host, and from a device buffer of a coupled model
        full = (np.arange(rows)[:, None] * 4096 + np.arange(P)[None, :]).astype(dtype)
        d.set_ring(name, full if rows > 1 else full[0])
        expect = R.columns_from_ring_field(full, mask)
        check_gathered(d, name, expect, Nz)
        back = (np.arange(rows)[:, None] * 4096 + (P - 1 - np.arange(P))[None, :]).astype(dtype)
        src = torch.as_tensor(back, device=dev)
        torch.cuda.synchronize()
        d.gather_ring_from(name, src.data_ptr())
        check_gathered(d, name, R.columns_from_ring_field(back, mask), Nz)
        scrub(d)
        assert np.array_equal(np.atleast_2d(d.get_ring(name, fill=fill)), np.where(mask[None, :], back, dtype(fill))), name


def test_ring_grid_and_row_refusals():
    Nh, Nz = 5, 3
    import torch
    d = fresh_state(Nh, Nz, np.float64)
    good = np.array([0, 2, 4, 6, 8])
    raises(EINVAL, "trm_set_ring_grid: bad argument", lambda: d.set_ring_grid(Nh - 1, good))                 # num_points < Nh
    for bad in ([0, 2, 4, 6, 9], [-1, 2, 4, 6, 8], [0, 2, 2, 6, 8], [0, 4, 2, 6, 8]):                        # = num_points, negative, repeated, unordered
        raises(EINVAL, "strictly increasing", lambda: d.set_ring_grid(9, np.array(bad)))
    d.set_ring_grid(9, good)
    T, K = encoded(Nz, Nh, np.float64), encoded(Nz + 1, Nh, np.float64)
    d.set("temperature", T)
    d.set("hydraulic_conductivity", K)
    out_of_range = [("temperature", -1, 1), ("temperature", Nz, 1), ("temperature", Nz - 1, 2), ("temperature", 0, Nz + 1), ("temperature", 0, 0),
                    ("hydraulic_conductivity", -1, 2), ("hydraulic_conductivity", Nz + 1, 1), ("hydraulic_conductivity", Nz, 2),
                    ("hydraulic_conductivity", 0, Nz + 2), ("water_table", 1, 1), ("water_table", 0, 2), ("water_table", -1, 1)]
    for name, row0, nrows in out_of_range:
        raises(EINVAL, "rows out of range", lambda: d.get_rows(name, row0, nrows))
        raises(EINVAL, "rows out of range", lambda: d.get_ring(name, row0=row0, nrows=nrows))
        buf = torch.zeros((max(nrows, 1), 9), dtype=torch.float64, device="cuda")
        raises(EINVAL, "rows out of range", lambda: d.scatter_ring_to(name, buf.data_ptr(), row0=row0, nrows=nrows))
    # the rows next to every refused window are served
    assert np.array_equal(d.get_rows("temperature", Nz - 1, 1), T[-1:]) and np.array_equal(d.get_rows("hydraulic_conductivity", Nz, 1), K[-1:])
    assert np.array_equal(d.get_ring("hydraulic_conductivity", fill=0.0, row0=Nz - 1, nrows=2), R.ring_field_from_columns(K[-2:], np.arange(9) % 2 == 0, 0.0))


# ---- 3. reductions against a high-precision reference -----------------------------------------------------------------------------
def decades(rng, shape, dtype):
    """both signs, magnitudes over twelve decades"""
    return (rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-6.0, 6.0, size=shape)).astype(dtype)


REDUCED = (("temperature", lambda Nz: Nz), ("hydraulic_conductivity", lambda Nz: Nz + 1), ("water_table", lambda Nz: 1))


def upload(d, name, a):
    d.set(name, a if a.shape[0] > 1 else a[0])


def context_dzc(d, dtype):
    """the layer thicknesses as the context holds them: rounded to its precision"""
    dzc = d._grid_arrays()["dzc"]
    return dzc.astype(dtype).astype(np.float64)


def fsum_longdouble(p):
    """math.fsum of np.longdouble terms without rounding them to double first: each is split into two doubles exactly"""
    hi = p.astype(np.float64)
    lo = (p - hi.astype(np.longdouble)).astype(np.float64)
    assert np.array_equal(hi.astype(np.longdouble) + lo.astype(np.longdouble), p)
    return math.fsum(hi.ravel().tolist() + lo.ravel().tolist())


def twice(d, name, op):
    a, b = d.reduce(name, op), d.reduce(name, op)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (name, op)         # deterministic: the same bits
    return a


@pytest.mark.parametrize("shape", SHAPES + [LARGE], ids=shape_id)
def test_reductions_against_fsum(shape):
    Nh, Nz, dtype = shape
    d = state_of(shape)
    rng = np.random.default_rng([4, Nh, Nz, np.dtype(dtype).itemsize])
    for name, rows_of in REDUCED:
        rows = rows_of(Nz)
        upload(d, name, decades(rng, (rows, Nh), dtype))
        x = np.atleast_2d(d.get(name)).astype(np.float64)                           # (fp32 converts to double exactly)
        assert x.shape == (rows, Nh) and np.isfinite(x).all()
        assert np.array_equal(twice(d, name, "min"), x.min(axis=1)), name
        assert np.array_equal(twice(d, name, "max"), x.max(axis=1)), name
        assert np.array_equal(twice(d, name, "hasnan"), np.zeros(rows)), name
        got = twice(d, name, "sum")
        worst = 0.0
        for r in range(rows):
            err = abs(got[r] - math.fsum(x[r].tolist()))
            bound = (Nh - 1) * U * math.fsum(np.abs(x[r]).tolist())
            worst = max(worst, err / bound if bound > 0 else 0.0)
            assert err <= bound, (name, r, err, bound)
        print(f"\nratio sum {shape_id(shape)} {name}: {worst:.4f}")
        if rows == Nz:
            dzc = context_dzc(d, dtype)
            p = x.astype(np.longdouble) * dzc.astype(np.longdouble)[:, None]
            got = twice(d, name, "volume_integral_z")
            assert got.shape == (1,)
            err = abs(np.longdouble(got[0]) - np.longdouble(fsum_longdouble(p)))
            bound = (Nz * Nh) * U * fsum_longdouble(np.abs(p))
            print(f"ratio volume_integral_z {shape_id(shape)} {name}: {float(err / bound):.4f}")
            assert err <= bound, (name, float(err), float(bound))
        else:
            raises(EINVAL, "cell-centred 3-D field", lambda: d.reduce(name, "volume_integral_z"))


def test_closed_form_reductions_past_one_stride_trip():
    """Nh = 65 536 + 257: 256 blocks of 256 threads, columns 65 536 ... 65 792 in the second trip of the loop (block 0 whole, block 1 one
    lane).  (k - 1) * 2^22 + i is exact in fp32 and its sums are exact in double: a column read twice or not at all shows."""
    Nh, Nz, dtype = LARGE
    d = state_of(LARGE)
    for name, rows in (("temperature", Nz), ("hydraulic_conductivity", Nz + 1)):
        host = encoded_large(rows, Nh, dtype)
        assert np.unique(host).size == host.size
        d.set(name, host)
        assert np.array_equal(d.get(name), host)
        check_closed_form_reductions(d, name, rows, Nh, lambda k: (k - 1) * 2.0 ** 22)
    wt = encoded_large(3, Nh, dtype)[2]
    d.set("water_table", wt)
    check_closed_form_reductions(d, "water_table", 1, Nh, lambda k: k + 2.0 ** 22)


def nan_columns(Nh):
    """column 0, the last one, both sides of the wave seam (63 | 64), of the block seam (255 | 256) and -- where the stride loop runs a
    second trip -- its first column, the last column of its full block, the first and last of its partial block"""
    return sorted({c for c in (0, Nh - 1, 63, 64, 255, 256, 65535, 65536, 65536 + 255, 65536 + 256) if c < Nh})


NAN_SHAPES = [(1, 2, np.float64), (33, 33, np.float32), (65, 64, np.float64), (65, 64, np.float32), (257, 65, np.float64),
              (257, 65, np.float32), (31, 97, np.float64), LARGE]


@pytest.mark.parametrize("shape", NAN_SHAPES, ids=shape_id)
def test_one_nan_reaches_its_row_and_no_other(shape):
    Nh, Nz, dtype = shape
    d = state_of(shape)
    rng = np.random.default_rng([5, Nh, Nz, np.dtype(dtype).itemsize])
    for name, rows_of in REDUCED:
        rows = rows_of(Nz)
        clean = decades(rng, (rows, Nh), dtype)
        upload(d, name, clean)
        before = {op: d.reduce(name, op) for op in OPS[:4]}
        assert not before["hasnan"].any()
        if rows == Nz:
            assert np.isfinite(d.reduce(name, "volume_integral_z")[0])
        for row in sorted({0, rows // 2, rows - 1}):       # (row Nz of the face field: the top face in its own buffer, stride 1)
            for col in nan_columns(Nh):
                a = clean.copy()
                a[row, col] = np.nan
                upload(d, name, a)
                others = np.arange(rows) != row
                for op in ("min", "max", "sum"):
                    got = d.reduce(name, op)
                    assert np.isnan(got[row]), (name, op, row, col)
                    assert np.array_equal(got[others].view(np.uint64), before[op][others].view(np.uint64)), (name, op, row, col)
                assert np.array_equal(d.reduce(name, "hasnan"), (~others).astype(np.float64)), (name, row, col)
                if rows == Nz:
                    assert np.isnan(d.reduce(name, "volume_integral_z")[0]), (name, row, col)


INF_SHAPES = [(33, 33, np.float32), (257, 65, np.float64), (63, 32, np.float64), LARGE]


@pytest.mark.parametrize("shape", INF_SHAPES, ids=shape_id)
def test_infinities_are_values_not_nans(shape):
    """A row of +Inf sums to +Inf; a row that mixes +Inf and -Inf sums to NaN (Inf - Inf) without holding one: hasnan stays 0."""
    Nh, Nz, dtype = shape
    d = state_of(shape)
    rng = np.random.default_rng([6, Nh, Nz])
    for name, rows_of in REDUCED[:2]:
        rows = rows_of(Nz)
        a = decades(rng, (rows, Nh), dtype)
        a[0, :] = np.inf
        a[rows - 1, :] = np.inf
        a[rows - 1, Nh // 2] = -np.inf                      # (the last column of the second trip's full block in the large context: below)
        if Nh > 65536:
            a[rows - 1, Nh // 2] = np.inf
            a[rows - 1, 65536 + 255] = -np.inf
        upload(d, name, a)
        x = a.astype(np.float64)
        assert np.array_equal(d.reduce(name, "hasnan"), np.zeros(rows)), name
        assert np.array_equal(d.reduce(name, "min"), x.min(axis=1)) and np.array_equal(d.reduce(name, "max"), x.max(axis=1)), name
        s = d.reduce(name, "sum")
        assert s[0] == np.inf and np.isnan(s[rows - 1]) and np.isfinite(s[1:rows - 1]).all(), (name, s[0], s[rows - 1])
        assert d.reduce(name, "min")[rows - 1] == -np.inf and d.reduce(name, "max")[rows - 1] == np.inf
        if rows == Nz:
            assert np.isnan(d.reduce(name, "volume_integral_z")[0])


ZERO_SHAPES = [(1, 2, np.float64), (33, 33, np.float64), (65, 64, np.float32), (257, 65, np.float64), (257, 65, np.float32), LARGE]


@pytest.mark.parametrize("shape", ZERO_SHAPES, ids=shape_id)
def test_the_sign_of_a_zero_minimum_and_maximum(shape):
    """Julia: minimum([0.0, -0.0]) === -0.0, maximum([-0.0, 0.0]) === 0.0, wherever the other zero sits in the fold."""
    Nh, Nz, dtype = shape
    d = state_of(shape)
    places = sorted({c for c in (0, Nh // 2, Nh - 1, 63, 64, 255, 256, 65536, 65536 + 256) if c < Nh})
    for name, rows_of in REDUCED:
        rows = rows_of(Nz)
        for row in sorted({0, rows - 1}):
            for col in places:
                for lone in (-0.0, 0.0):                    # one zero of this sign among zeros of the other
                    a = np.ones((rows, Nh), dtype=dtype)
                    a[row, :] = -lone
                    a[row, col] = lone
                    upload(d, name, a)
                    lo, hi = d.reduce(name, "min"), d.reduce(name, "max")
                    both = Nh > 1
                    assert lo[row] == 0 and hi[row] == 0
                    assert np.signbit(lo[row]) == (both or np.signbit(lone)), (name, row, col, lone)
                    assert np.signbit(hi[row]) == (not both and np.signbit(lone)), (name, row, col, lone)
                    others = np.arange(rows) != row
                    assert (lo[others] == 1).all() and (hi[others] == 1).all()
            a = np.ones((rows, Nh), dtype=dtype)
            a[row, :] = -0.0                                # nothing but negative zeros: the maximum is one of them
            upload(d, name, a)
            assert np.signbit(d.reduce(name, "max")[row]) and np.signbit(d.reduce(name, "min")[row]), (name, row)


def test_host_fold_of_two_shards():
    """trm_reduce_global_all without communicators (two contexts on one device): a NaN in one shard only reaches the global minimum
    and maximum; zeros of both signs in different shards give -0 / +0 in either order of the shards."""
    Nh, Nz = 65, 33
    a, b = fresh_state(Nh, Nz, np.float64), fresh_state(Nh, Nz, np.float64)
    rng = np.random.default_rng(7)
    A, B = decades(rng, (Nz, Nh), np.float64), decades(rng, (Nz, Nh), np.float64)
    A[2, :] = 0.0
    B[2, :] = 0.0
    B[2, 64] = -0.0
    A[5, :] = -0.0
    B[5, :] = -0.0
    A[5, 0] = 0.0
    B[7, 64] = np.nan
    a.set("temperature", A)
    b.set("temperature", B)
    whole = np.concatenate([A, B], axis=1)
    for group in (trm.DeviceGroup([a, b]), trm.DeviceGroup([b, a])):
        lo, hi, s, has = (group.reduce_global("temperature", op) for op in ("min", "max", "sum", "hasnan"))
        assert np.isnan(lo[7]) and np.isnan(hi[7]) and np.isnan(s[7])
        assert np.array_equal(has, (np.arange(Nz) == 7).astype(np.float64))
        ok = np.arange(Nz) != 7
        assert np.array_equal(lo[ok], whole.min(axis=1)[ok]) and np.array_equal(hi[ok], whole.max(axis=1)[ok])
        for row in (2, 5):
            assert lo[row] == 0 and hi[row] == 0 and np.signbit(lo[row]) and not np.signbit(hi[row]), row
        assert np.isnan(group.reduce_global("temperature", "volume_integral_z")[0])
    assert np.isnan(b.reduce("temperature", "min")[7]) and not np.isnan(a.reduce("temperature", "min")).any()


def test_tendencies_stay_stale_for_reductions():
    d = fresh_state(33, 33, np.float64, initializers=dict(temperature=2.0, saturation_water_ice=0.5),
                    boundary_conditions=trm.PrescribedSurfaceTemperature("T_ub", -3.0))
    d.step(60.0, 2, finalize=False)
    for name in ("tend_internal_energy", "tend_saturation_water_ice", "tend_surface_excess_water"):
        for op in OPS:
            raises(ESTALE, "not materialised", lambda: d.reduce(name, op))
    assert np.isfinite(d.reduce("temperature", "sum")).all()
    d.step(60.0, 1, finalize=True)
    assert np.isfinite(d.reduce("tend_internal_energy", "sum")).all() and d.reduce("tend_internal_energy", "hasnan").sum() == 0


# ---- 4. the refusals ----------------------------------------------------------------------------------------------------------------
LAZY = ("plant_available_water", "root_fraction")
ONLY_AFTER = "exists only after trm_set_vegetation"


def test_unallocated_vegetation_fields_are_refused_before_any_launch():
    """plant_available_water and root_fraction are null until trm_set_vegetation: every reader refuses them by name -- none launches."""
    Nh, Nz = 65, 33
    d = trm.DeviceState(trm.ColumnGrid(trm.ExponentialSpacing(N=Nz), num_columns=Nh), trm._capi.default_params())
    group = trm.DeviceGroup([d])
    for name in LAZY:
        for op in OPS:
            raises(EINVAL, "trm_reduce: the field " + ONLY_AFTER, lambda: d.reduce(name, op))
            raises(EINVAL, "trm_reduce: the field " + ONLY_AFTER, lambda: group.reduce_global(name, op))
            raises(EINVAL, "trm_reduce: the field " + ONLY_AFTER, lambda: d.reduce_global(name, op))
        raises(EINVAL, "trm_field_device_ptr: the field " + ONLY_AFTER, lambda: d.device_array(name))
        raises(EINVAL, "trm_stage_field_device_ptr: the field " + ONLY_AFTER, lambda: d.stage_device_array(name))
        raises(EINVAL, ONLY_AFTER, lambda: d.get(name))
        raises(EINVAL, "bad argument", lambda: d.get_rows(name, 0, 1))
    assert d.status() == 0 and np.array_equal(d.reduce("temperature", "hasnan"), np.zeros(Nz))     # the context is as it was
    d.set_vegetation(trm._capi.default_vegetation_params(), "standalone")
    for name in LAZY:
        x = d.get(name).astype(np.float64)
        assert np.array_equal(d.reduce(name, "min"), x.min(axis=1)) and np.array_equal(d.reduce(name, "max"), x.max(axis=1))
        assert np.array_equal(group.reduce_global(name, "max"), x.max(axis=1))
        assert np.array_equal(d.reduce(name, "hasnan"), np.zeros(Nz))
        assert np.allclose(d.reduce(name, "sum"), x.sum(axis=1), rtol=1e-13, atol=0)
        assert np.isfinite(d.reduce(name, "volume_integral_z")[0])
        assert np.array_equal(view_to_host(d, name)[:, :Nz].T, x)
    assert d.get("root_fraction").max() > 0
    d.close()


def test_one_layer_grids_do_not_exist():
    """VOLUME_INTEGRAL_Z is guarded by the kind of the field, not by its row count alone, which would let every 2-D field of a
    one-layer grid through; trm_create refuses such a grid in the first place, so the refusal shows on the smallest grid there is."""
    with pytest.raises(trm.TerrariumHipError, match="num_layers must be >= 2"):
        trm.DeviceState(trm.ColumnGrid(trm.UniformSpacing(dz=0.1, N=1), 4), trm._capi.default_params())
    d = state_of((1, 2, np.float64))
    for name in ("water_table", "surface_excess_water", "air_temperature", "hydraulic_conductivity"):
        raises(EINVAL, "cell-centred 3-D field", lambda: d.reduce(name, "volume_integral_z"))
    out = np.zeros(2)
    raises(EINVAL, "unknown reduction op", lambda: d._check(d._lib.trm_reduce(d._ctx, trm._capi.FIELD["temperature"], 5, out.ctypes.data), "trm_reduce"))
