"""Cases, inputs and reference of tests/test_vegetation_edges_host.py and tests/test_gpu_vegetation_edges.py: plant available
water (FieldCapacityLimitedPAW, plant_available_water.jl:36-94) and its root-weighted column sum, the soil moisture limiting
factor, at the edges of the device's block layout -- 64 columns per workgroup, level pitch 32 / 64, one thread per column
beyond 64 levels -- with inputs that differ from cell to cell, so that a wrong column or level index cannot hide.

Pure numpy: the reference is a restatement in the case's own dtype, every operation rounded to it, of

    water = (sat * por) * liq
    W     = max(min(1, (water - wilting_point) / (field_capacity - wilting_point)), 0)
    term  = (W * root_fraction / dz) * dz
    soil_moisture_limiting_factor = term[0] + term[1] + ...        sequentially, from the bottom cell up (Oceananigans' Integral)

which the oracle (tests/test_vegetation_edges_host.py) and the device (tests/test_gpu_vegetation_edges.py) must both equal bit
for bit: every operation is a correctly rounded IEEE operation in either."""
import functools

import numpy as np

# pitch 32 with and without padding levels, the first depth of pitch 64, pitch 64 full, the first depth of the
# one-thread-per-column kernel, a wide column
DEPTHS = (2, 31, 32, 33, 63, 64, 65, 129)
# one column, a workgroup one short of full, exactly full, full plus a one-column tail, two full plus a two-column tail
WIDTHS = (1, 63, 64, 65, 130)
DTYPES = (np.float64, np.float32)
CASES = [(Nz, Nh, dt) for dt in DTYPES for Nz in DEPTHS for Nh in WIDTHS]
case_id = lambda c: f"Nz{c[0]}-Nh{c[1]}-{np.dtype(c[2]).name}"

# (the first seed from 20261020 up at which every case, standalone and coupled, meets input_conditions below: a single column of
# 31-33 cells drawn this way falls short of a quarter of its cells inside the ramp about one time in five)
SEED = 20261026
POR_MINERAL, POR_ORGANIC, RHO_SOC, RHO_ORG = 0.49, 0.9, 0.0, 1300.0      # the default soil (oracle.default_params)
WILTING_POINT, FIELD_CAPACITY = 0.05, 0.25                               # oracle.default_vegetation_params
DZ_TOP = 0.05                                                            # [m] thickness of the surface cell
RATIO = 1.015                                                            # thickness of a cell / thickness of the cell above it


def thickness(Nz):
    """Geometric PrescribedSpacing, index 0 = the SURFACE cell (the thinnest): dz and 1 / dz differ from level to level.  The surface
    cell is 5 cm as in the reference's default grids (a much thinner or thicker one makes the explicit coupled step unstable within
    the four steps of the GPU test -- in the oracle as on the device); 129 levels reach 19.4 m, where the root density
    (7 exp(7 z) + 2 exp(2 z)) / 2 is still a normal number in fp32."""
    return DZ_TOP * RATIO ** np.arange(Nz, dtype=np.float64)


def porosity(dtype):
    """homogeneous_strat.jl:34-61 in `dtype`"""
    nf = np.dtype(dtype).type
    org = nf(RHO_SOC) / ((nf(1) - nf(POR_ORGANIC)) * nf(RHO_ORG))
    return (nf(1) - org) * nf(POR_MINERAL) + org * nf(POR_ORGANIC)


def _draw(rng, Nz, Nh, dtype):
    """saturation uniform in [0.05, 1] per cell, rounded to dtype.  The TOP cell of every column (the largest root fraction) is
    drawn inside the ramp instead, sat in [0.12, 0.5): its term is then a continuous random number that dominates the column sum,
    which keeps the sums of any two columns apart even in a two-level column."""
    sat = rng.uniform(0.05, 1.0, (Nz, Nh))
    sat[-1] = rng.uniform(0.12, 0.5, Nh)
    return sat.astype(dtype)


@functools.lru_cache(maxsize=None)
def inputs(Nz, Nh, dtype):
    """(saturation_water_ice, liquid_water_fraction) [Nz][Nh], k = 0 the bottom cell, in `dtype`.  liquid fraction: 1 in about 70 %
    of the cells, uniform in (0, 1) in about 20 %, 0 in about 10 %; 1 in the top cell."""
    rng = np.random.default_rng([SEED, Nz, Nh, np.dtype(dtype).itemsize])
    sat = _draw(rng, Nz, Nh, dtype)
    u = rng.uniform(0.0, 1.0, (Nz, Nh))
    partial = rng.uniform(0.0, 1.0, (Nz, Nh)).astype(dtype)
    partial = np.clip(partial, np.finfo(dtype).eps, 1 - np.finfo(dtype).eps).astype(dtype)      # the OPEN interval after rounding
    liq = np.where(u < 0.7, 1.0, np.where(u < 0.9, partial, 0.0)).astype(dtype)
    liq[-1] = 1
    sat.setflags(write=False)
    liq.setflags(write=False)
    return sat, liq


@functools.lru_cache(maxsize=None)
def coupled_initial_state(Nz, Nh, dtype):
    """Initial (saturation_water_ice, temperature) of the coupled LandModel at a case's shape: the saturation drawn as above, the
    temperature uniform in [-2, 6) degC per cell (the model derives the liquid fraction: about a quarter of the cells start
    frozen), 1 to 6 degC in the top cell."""
    rng = np.random.default_rng([SEED + 1, Nz, Nh, np.dtype(dtype).itemsize])
    sat = _draw(rng, Nz, Nh, dtype)
    T = rng.uniform(-2.0, 6.0, (Nz, Nh))
    T[-1] = rng.uniform(1.0, 6.0, Nh)
    T = T.astype(dtype)
    sat.setflags(write=False)
    T.setflags(write=False)
    return sat, T


def _jl_min(x, y):
    d = x - y
    return np.where(np.isnan(x) | np.isnan(y), d, np.where(np.signbit(d), x, y))


def _jl_max(x, y):
    d = x - y
    return np.where(np.isnan(x) | np.isnan(y), d, np.where(np.signbit(d), y, x))


def restate(sat, liq, root_fraction, dz, dtype):
    """(plant_available_water [Nz][Nh], terms [Nz][Nh], soil_moisture_limiting_factor [Nh]) in `dtype`.  root_fraction: [Nz][Nh]
    or [Nz]; dz: [Nz], bottom cell first."""
    nf = np.dtype(dtype).type
    sat, liq = np.asarray(sat), np.asarray(liq)
    assert sat.dtype == liq.dtype == np.dtype(dtype) and sat.shape == liq.shape
    rf = np.asarray(root_fraction)
    dz = np.asarray(dz)
    assert rf.dtype == dz.dtype == np.dtype(dtype)
    rf = rf if rf.ndim == 2 else rf[:, None]
    dz = dz[:, None]
    wp, fc = nf(WILTING_POINT), nf(FIELD_CAPACITY)
    water = (sat * porosity(dtype)) * liq
    paw = _jl_max(_jl_min(nf(1), (water - wp) / (fc - wp)), nf(0)).astype(dtype)
    terms = ((paw * rf / dz) * dz).astype(dtype)
    acc = np.zeros(sat.shape[1], dtype=dtype)
    for k in range(sat.shape[0]):
        acc = acc + terms[k]
    assert paw.dtype == terms.dtype == acc.dtype == np.dtype(dtype)
    return paw, terms, acc


def bits(a):
    """the array's bit patterns (so that -0.0 != +0.0 and NaN == NaN)"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def input_conditions(paw, terms, smlf):
    """The conditions that make a wrong index visible, as a list of messages (empty = all hold):
      * at least a quarter of the cells lie inside the ramp, 0 < W < 1;
      * both clamps occur (cases of at least 31 cells; a smaller one cannot hold both beside its top cell);
      * no two columns share a soil moisture limiting factor;
      * no two levels of a column share a NON-ZERO term.  (A cell without available water contributes an exact zero whatever its
        level, and with a tenth of the cells frozen every deep column has several; the per-cell comparison of W covers them.)"""
    out = []
    inside = (paw > 0) & (paw < 1)
    if inside.mean() < 0.25:
        out.append(f"only {inside.mean():.2f} of the cells inside the ramp")
    if paw.size >= 31 and not (np.any(paw == 0) and np.any(paw == 1)):
        out.append("a clamp does not occur")
    if np.unique(bits(smlf)).size != smlf.size:
        out.append("two columns share a soil moisture limiting factor")
    for i in range(terms.shape[1]):
        t = terms[:, i][terms[:, i] != 0]
        if np.unique(bits(t)).size != t.size:
            out.append(f"column {i}: two levels share a term")
            break
    return out
