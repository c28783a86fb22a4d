"""The accuracy metric of tests/test_accuracy_host.py and tests/test_gpu_accuracy.py: an evaluation in precision NF (the
device, or the same-precision oracle) measured per field against the WIDE oracle -- the same model, parameters, grid and
inputs, all rounded to NF first, evaluated in long double (oracle.Oracle(dtype=np.longdouble, model=NF)).

For a field f with reference values ref:

    S_f   = max |ref|                                   the field's own scale
    e(x)  = max |x - ref| / S_f                         error in units of that scale
    r(x)  = max |x - ref| / |ref|  over ref != 0        per-cell relative error, REL_FIELDS only (sign-definite fields whose
                                                        values span decades, where S_f says nothing about the small cells)

and the assertion on the tested values `dev`, with `orc` the same-precision oracle:

    e(dev) <= M * e(orc) + eps(NF)        r(dev) <= M * r(orc) + eps(NF)

The yardstick is the reference side alone: e(orc) is what one plain NF evaluation of the same formulas loses against the
wide one, M the factor a second, independently rounded NF evaluation may be worse by, and eps(NF) the floor (the value is
stored in NF: rounding the stored value alone costs up to eps(NF) / 2 of the scale, and both sides pay it).  Where S_f == 0
the tested field must be all zero; finite and non-finite cells must coincide.

REGIME FLIPS.  A cell that crosses a threshold (freezing, the saturation repair, the water table) in one evaluation and not
in the other differs by O(1) without any arithmetic being wrong.  Cells whose regime -- the liquid-fraction branch and the
saturation clamp -- differs between `dev` and `ref` are left out, counted and printed; more than MAX_LEFT_OUT of a field's
cells left out fails."""
import numpy as np

import oracle
import workloads as W

M_CAP = 8                # the issue's cap on M (see tests/test_gpu_accuracy.py for the measured M)
MAX_LEFT_OUT = 1.0e-3    # fraction of a field's cells that may be left out for a regime flip
# (transpiration and evaporation_canopy: sign-definite under the 0.1 Pa floor of the vapour pressure deficit, and spanning decades
# through the floor of the canopy conductance; tests/test_accuracy_host.py checks that their r_orc is rounding-sized in fp32)
REL_FIELDS = ("hydraulic_conductivity", "pressure_head", "saturation_water_ice", "evaporation_ground", "infiltration",
              "transpiration", "evaporation_canopy")
TENDENCIES = ("tend_internal_energy", "tend_saturation_water_ice", "tend_surface_excess_water")


def wide_skip_reason():
    """None where the wide oracle is usable, else why not."""
    nmant = np.finfo(np.longdouble).nmant
    if nmant < 63:
        return f"np.longdouble has {nmant + 1} significand bits here: no format wider than float64 to measure against"
    if not oracle.wide_available():
        return "the C library's long double is not numpy's longdouble here"
    return None


def eps(dtype):
    return float(np.finfo(np.dtype(dtype)).eps)


# ---- the three evaluations from identical inputs --------------------------------------------------------------------------
def rounded_workload(w):
    """The workload with every array input rounded to its dtype, so that the device, the oracle and the wide oracle start from
    identical values (each of them would round on its own; this makes it explicit)."""
    nf = w["dtype"]
    r = lambda v: np.asarray(v, dtype=nf) if np.ndim(v) else v
    return dict(w, fields={k: r(v) for k, v in w["fields"].items()}, bcs={k: (kind, r(v)) for k, (kind, v) in w["bcs"].items()},
                inputs={k: r(v) for k, v in w["inputs"].items()})


def setup_oracle(w, wide=False, dx=0.0):
    """W.setup_oracle with the arithmetic type chosen: the workload's own dtype, or long double with that dtype as the model."""
    p = oracle.default_params(**w["params"])
    if wide:
        o = oracle.Oracle(w["Nh"], w["thickness"], p, dtype=np.longdouble, model=w["dtype"], dx=dx)
    else:
        o = oracle.Oracle(w["Nh"], w["thickness"], p, dtype=w["dtype"], dx=dx)
    if w.get("vegetation"):
        o.enable_vegetation()
    for name, v in w["fields"].items():
        o.set(name, v)
    for (var, side), (kind, value) in w["bcs"].items():
        o.set_bc(var, side, kind, value)
    for name, v in w["inputs"].items():
        o.set(name, v)
    o.initialize()
    return o


def run_oracle(o, dt, nsteps, heun=False):
    """run!(steps = nsteps): compute_auxiliary! once, after the last step"""
    for n in range(nsteps):
        (o.timestep_heun if heun else o.timestep)(dt, n == nsteps - 1)


def field_names(w, tendencies=True):
    names = list(W.compared_fields(w))
    if tendencies:
        names += [t for t in TENDENCIES if w["config"] != "heat" or t == "tend_internal_energy"]
    return names


def fields_of(source, names):
    """{name: array} from an oracle or a device state"""
    return {n: np.asarray(source.get(n)) for n in names}


# ---- the metric -----------------------------------------------------------------------------------------------------------
def _regime(fields):
    """per-cell regime code (Nz, Nh) or None when the fields that define it are absent"""
    if "liquid_water_fraction" not in fields:
        return None
    liq = np.asarray(fields["liquid_water_fraction"])
    code = np.where(liq >= 1, 2, np.where(liq <= 0, 0, 1))
    if "saturation_water_ice" in fields:
        sat = np.asarray(fields["saturation_water_ice"])
        code = code + 3 * np.where(sat >= 1, 2, np.where(sat <= 0, 0, 1))
    return code


def left_out_masks(dev, ref):
    """Cells whose regime differs between dev and ref, as masks for the three field shapes: cell centres (Nz, Nh), faces
    (Nz + 1, Nh: a face belongs to the cells either side of it, the top face to the top cell) and columns (Nh,: a surface or
    column quantity depends on the whole column)."""
    a, b = _regime(dev), _regime(ref)
    if a is None or b is None:
        return None
    flip = a != b
    face = np.zeros((flip.shape[0] + 1,) + flip.shape[1:], dtype=bool)
    face[:-1] |= flip
    face[1:] |= flip
    return dict(cell=flip, face=face, column=flip.any(axis=0))


def measure(x, ref, left_out=None):
    """(S_f, e, r, n_left_out) of values x against ref (long double); r over the cells with ref != 0.  Non-finite cells are
    the caller's to compare; they do not enter."""
    ref = np.asarray(ref, dtype=np.longdouble)
    x = np.asarray(x).astype(np.longdouble)
    keep = np.isfinite(ref) & np.isfinite(x)
    n_out = 0
    if left_out is not None:
        n_out = int(np.count_nonzero(left_out & keep))
        keep &= ~left_out
    if not keep.any():
        return 0.0, 0.0, 0.0, n_out
    S = float(np.max(np.abs(ref[keep])))
    d = np.abs(x[keep] - ref[keep])
    if S == 0.0:
        return 0.0, (0.0 if not d.any() else np.inf), 0.0, n_out
    nz = ref[keep] != 0
    r = float(np.max(d[nz] / np.abs(ref[keep][nz]))) if nz.any() else 0.0
    return S, float(np.max(d) / S), r, n_out


def _mask_for(name, shape, masks):
    if masks is None:
        return None
    for m in masks.values():
        if m.shape == tuple(shape):
            return m
    return None


def compare(dev, orc, ref, names, nf, label="", exclude_flips=True):
    """One row per field: dict(name, S, e_orc, e_dev, r_orc, r_dev, ratio_e, ratio_r, left_out, cells, bad_nonfinite).
    ratio_* = (err_dev - eps) / err_orc, the factor M has to cover (0 where the device is inside the floor, inf where the
    oracle's error is zero and the device's is above the floor).  Prints the rows (pytest -s)."""
    e0 = eps(nf)
    masks = left_out_masks(dev, ref) if exclude_flips else None
    rows = []
    for n in names:
        d, o, r = np.asarray(dev[n]), np.asarray(orc[n]), np.asarray(ref[n])
        assert d.shape == o.shape == r.shape, (n, d.shape, o.shape, r.shape)
        m = _mask_for(n, r.shape, masks)
        S, e_orc, r_orc, _ = measure(o, r)
        _, e_dev, r_dev, n_out = measure(d, r, m)
        considered = ~m if m is not None else np.ones(r.shape, dtype=bool)
        bad = int(np.count_nonzero((np.isfinite(d) != np.isfinite(r)) & considered))
        ratio = lambda x_dev, x_orc: 0.0 if x_dev <= e0 else (np.inf if x_orc == 0 else (x_dev - e0) / x_orc)
        rel = n in REL_FIELDS
        rows.append(dict(name=n, S=S, e_orc=e_orc, e_dev=e_dev, r_orc=r_orc if rel else None, r_dev=r_dev if rel else None,
                         ratio_e=ratio(e_dev, e_orc), ratio_r=ratio(r_dev, r_orc) if rel else None, left_out=n_out, cells=r.size,
                         bad_nonfinite=bad, zero_scale=S == 0.0, dev_all_zero=not np.any(d[considered] != 0)))
    print(f"\n{label}  NF = {np.dtype(nf).name}  eps = {e0:.3e}")
    print(f"  {'field':<28}{'S_f':>11}{'e_orc':>11}{'e_dev':>11}{'ratio':>9}{'r_orc':>11}{'r_dev':>11}{'ratio':>9}{'left out':>10}")
    g = lambda v, f: f"{'-':>{int(f.split('.')[0])}}" if v is None else format(v, f)
    for q in rows:
        print(f"  {q['name']:<28}{q['S']:>11.3e}{q['e_orc']:>11.3e}{q['e_dev']:>11.3e}{q['ratio_e']:>9.3g}"
              f"{g(q['r_orc'], '11.3e')}{g(q['r_dev'], '11.3e')}{g(q['ratio_r'], '9.3g')}{q['left_out']:>6}/{q['cells']}")
    return rows


def violations(rows, nf, M):
    """The assertion, as a list of messages (empty = passes)."""
    e0 = eps(nf)
    out = []
    for q in rows:
        n = q["name"]
        if q["bad_nonfinite"]:
            out.append(f"{n}: {q['bad_nonfinite']} cells finite on one side only")
        if q["left_out"] > MAX_LEFT_OUT * q["cells"]:
            out.append(f"{n}: {q['left_out']} of {q['cells']} cells left out for a regime flip (> {MAX_LEFT_OUT:.1%})")
        if q["zero_scale"]:
            if not q["dev_all_zero"]:
                out.append(f"{n}: the reference is identically zero, the tested field is not")
            continue
        if not q["e_dev"] <= M * q["e_orc"] + e0:
            out.append(f"{n}: e_dev {q['e_dev']:.3e} > {M} * e_orc {q['e_orc']:.3e} + eps {e0:.1e}  (S_f {q['S']:.3e})")
        if q["r_dev"] is not None and not q["r_dev"] <= M * q["r_orc"] + e0:
            out.append(f"{n}: r_dev {q['r_dev']:.3e} > {M} * r_orc {q['r_orc']:.3e} + eps {e0:.1e}")
    return out


def old_metric(x, orc):
    """max |x - orc| / max(1, |orc|): what the tolerance tests assert (1e-4 in fp32, 1e-10 in fp64)"""
    a, b = np.asarray(x, dtype=np.float64), np.asarray(orc, dtype=np.float64)
    return float(np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


# ---- the cases ------------------------------------------------------------------------------------------------------------
def small_columns(n, name="N72"):
    lat, lon = W.columns_from_mask(name)
    sel = np.linspace(0, lat.size - 1, n).astype(int)
    return lat[sel], lon[sel]


def sample_workload(w, sel):
    ws = dict(w)
    ws["Nh"] = sel.size
    for key in ("lat", "lon", "T0", "u"):
        ws[key] = w[key][sel]
    ws["fields"] = {k: (v[..., sel] if np.ndim(v) else v) for k, v in w["fields"].items()}
    ws["bcs"] = {k: (kind, (val[sel] if np.ndim(val) else val)) for k, (kind, val) in w["bcs"].items()}
    ws["inputs"] = {k: (v[sel] if np.ndim(v) else v) for k, v in w["inputs"].items()}
    return ws


class Case:
    """One workload of the accuracy suite.  `columns`: ("N72", n) = n columns spread over the N72 mask, ("N145",) = the whole
    N145 mask and ("synthetic", n) = n synthetic columns -- the last two run at full size on the device and are measured on
    `sample()`'s columns, the oracles running those columns alone with the full grid's dx."""

    def __init__(self, config, hydraulics, dtype, Nz, nsteps, columns, heun=False, params=None, tag="", sat_scale=None):
        self.config, self.hydraulics, self.dtype, self.Nz, self.nsteps = config, hydraulics, np.dtype(dtype), Nz, nsteps
        self.columns, self.heun, self.params, self.tag = columns, heun, dict(params or {}), tag
        self.sat_scale = sat_scale      # the workload's initial saturation times this factor (clipped to [0.05, 1] again)

    @property
    def id(self):
        p = "".join(f"-{k}={v:g}" for k, v in self.params.items())
        cols = self.columns[0] + (str(self.columns[1]) if len(self.columns) > 1 else "")
        return f"{self.config}-{self.hydraulics}-{self.dtype.name}-Nz{self.Nz}-{cols}-{'heun' if self.heun else 'euler'}{p}{self.tag}"

    def full_size(self):
        return self.columns[0] != "N72"

    def workload(self):
        """the workload as the device runs it (full size), inputs rounded to the case's dtype"""
        if self.columns[0] == "N72":
            lat, lon = small_columns(self.columns[1])
        elif self.columns[0] == "N145":
            lat, lon = W.columns_from_mask("N145")
        else:
            lat, lon = W.synthetic_columns(self.columns[1])
        w = W.make_workload(self.config, lat, lon, self.Nz, dtype=self.dtype, hydraulics=self.hydraulics)
        w["params"].update(self.params)
        if self.sat_scale is not None:
            w["fields"]["saturation_water_ice"] = np.clip(w["fields"]["saturation_water_ice"] * self.sat_scale, 0.05, 1.0)
        return rounded_workload(w)

    def sample(self, Nh):
        """columns the oracles run for a full-size case (tests/test_gpu_full_size.py's samples)"""
        if self.columns[0] == "N145":
            rng = np.random.default_rng(11)
            return np.unique(np.concatenate([[0, 1, 2, 31, 32, 63, 64, 65, Nh - 2, Nh - 1], rng.integers(0, Nh, 400)]))
        return np.unique(np.concatenate([[0, 1, 63, 64, 65, Nh - 2, Nh - 1], np.arange(0, Nh, Nh // 100)]))

    def oracle_workload(self, w):
        """(workload the oracles run, dx, selected columns or None)"""
        if not self.full_size():
            return w, 0.0, None
        sel = self.sample(w["Nh"])
        return sample_workload(w, sel), 1.0 / w["Nh"], sel

    def references(self, w):
        """(orc, ref, names, sel): fields of the same-precision and of the wide oracle after the case's steps"""
        ws, dx, sel = self.oracle_workload(w)
        names = field_names(ws)
        out = []
        for wide in (False, True):
            o = setup_oracle(ws, wide=wide, dx=dx)
            run_oracle(o, ws["dt"], self.nsteps, self.heun)
            assert o.status() == 0, (self.id, "wide" if wide else "same precision", o.status())
            out.append(fields_of(o, names))
        return out[0], out[1], names, sel


def _vg(alpha, n):
    return dict(swrc=1, unsat_k=1, vg_alpha=alpha, vg_n=n)


# The exponent classes of the run-time hydraulics (HYD_GENERIC; trm_device.hpp: make_pow_spec classifies each exponent, as
# the host forms it in NF, into INT, HALVES, THIRDS or GENERIC).  The sets are chosen by carrying out that arithmetic -- the
# quotients m = 1 - 1/n, -1/m, 1/n, n/(n+1), (n-1)/n, -1/lambda rounded in fp64 and in fp32 -- so that every class occurs on
# every exponent that can take it ("=" marks a class that holds in both precisions):
#   vg_n = 3     1/n = RN(1/3), (n-1)/n = RN(2/3): THIRDS =;  n/(n+1) = 3/4: GENERIC =;  -1/m = -1.4999999999999998 (fp64),
#                -1.5000001 (fp32): GENERIC -- m = 1 - RN(1/3) is not RN(2/3), so -3/2 is missed by one ulp
#   vg_n = 1.5   1/n = RN(2/3), (n-1)/n = RN(1/3): THIRDS =;  -1/m = -2.9999999999999996 / -3.0000002: GENERIC (one ulp off -3)
#   vg_n = 4     -1/m = RN(-4/3): THIRDS =;  1/n, (n-1)/n, n/(n+1): GENERIC =
#   vg_n = 1.7   GENERIC throughout = (a set of test_generic_hydraulics_parity)
#   vg_n = 1.4   -1/m = -7/2: HALVES in fp64 (fp32: -3.5000002, GENERIC)
#   vg_n = 2 with the linear conductivity      -1/m = -2: INT =;  1/n = 1/2: HALVES =   (retention only; set of that test)
#   vg_n = 2 under the BrooksCorey retention   n/(n+1) = RN(2/3): THIRDS =;  (n-1)/n = 1/2: HALVES =   (conductivity only; same)
#   bc_lambda = 0.25, 0.5   -1/lambda = -4, -2: INT =
#   bc_lambda = 0.4         -1/lambda = -5/2: HALVES =
#   bc_lambda = 0.3         -1/lambda = RN(-10/3): THIRDS =
#   bc_lambda = 0.35        -1/lambda = -2.857...: GENERIC =
# with the vg_alpha values of test_generic_hydraulics_parity (1.3, 2.0).  (n = 2 with both van Genuchten laws and
# lambda = 0.2 are the compile-time instances, covered by the other case lists.)
EXPONENT_SETS = [_vg(2.0, 3.0), _vg(1.3, 1.5), _vg(2.0, 4.0), _vg(1.3, 1.7), _vg(2.0, 1.4),
                 dict(swrc=1, unsat_k=0, vg_alpha=2.0, vg_n=2.0), dict(swrc=0, unsat_k=1, vg_alpha=2.0, vg_n=2.0),
                 dict(bc_lambda=0.25), dict(bc_lambda=0.5), dict(bc_lambda=0.4), dict(bc_lambda=0.3), dict(bc_lambda=0.35)]

f32, f64 = np.float32, np.float64
N72 = lambda n: ("N72", n)

# fp32: the three fp32 rows of test_gpu_parity.CASES, Euler and Heun (each with steps_per_launch 0 and 1 on the device)
FP32_PARITY = [Case(c, h, f32, nz, ns, N72(333), heun=heun)
               for (c, h, nz, ns) in (("heat", "default", 20, 100), ("richards", "default", 64, 100), ("land", "vg", 64, 50))
               for heun in (False, True)]
# deep (65-128 levels) and wide (129-256 levels) fp32 columns: the fp32 rows of test_gpu_deep_columns.CASES, and 250 levels
FP32_DEEP = [Case("richards", "default", f32, 100, 32, N72(50)), Case("land", "vg", f32, 66, 22, N72(41)),
             Case("heat", "default", f32, 128, 32, N72(9)),
             Case("richards", "default", f32, 250, 14, N72(15)), Case("land", "vg", f32, 250, 14, N72(10))]
# the C5 shard (fp32, 203 125 columns x 64 levels, 10 steps) on about 100 sampled columns with the full grid's dx
FP32_C5 = [Case("land", "default", f32, 64, 10, ("synthetic", 203125)), Case("land", "vg", f32, 64, 10, ("synthetic", 203125))]
# fp64 paths that are asserted with a tolerance today
FP64_TOL = [Case("richards", "vg", f64, 32, 100, N72(333))] + \
           [Case("land", h, f64, 32, 50, N72(333), heun=heun) for h in ("default", "vg") for heun in (False, True)] + \
           [Case("land", "default", f64, 96, 22, N72(130))]
FP64_N145 = [Case("land", "vg", f64, 32, 40, ("N145",)), Case("land", "default", f64, 32, 40, ("N145",))]
# every exponent class of the run-time hydraulics: richards, 32 levels, 60 steps, fp64 and fp32
EXPONENTS = [Case("richards", "default", nf, 32, 60, N72(60), params=ps) for nf in (f64, f32) for ps in EXPONENT_SETS]


# ---- vegetation ----------------------------------------------------------------------------------------
# The LandModel coupled to VegetationCarbon ("landveg": van Genuchten, 130 N72 columns, 20 steps of 0.05 s) at 20 levels (level
# pitch 32 of the cooperative 0-D kernel), 33 (pitch 64) and 70 (one thread per column, reference-order soil kernels), Euler and
# Heun, fp64 and fp32.  The workload's saturation keeps every unfrozen cell above the field capacity: plant available water is
# 1 or 0 throughout.  The "dry" variants scale the initial saturation by DRY so that (sat * porosity) * liq of the unfrozen
# cells lies inside the ramp between the wilting point 0.05 and the field capacity 0.25: porosity 0.49 and the workload's
# saturation in [0.76, 1] give a water content in [0.149, 0.196].
DRY = 0.4
VEG_COUPLED = [Case("landveg", "vg", nf, nz, 20, N72(130), heun=heun) for nf in (f64, f32) for nz in (20, 33, 70) for heun in (False, True)] + \
              [Case("landveg", "vg", nf, nz, 20, N72(130), heun=heun, sat_scale=DRY, tag="-dry") for nf in (f64, f32) for nz in (20, 33) for heun in (False, True)]
VEG_FIELDS = W.FIELDS_VEGETATION


class VegetationCase:
    """The standalone VegetationModel of tests/test_gpu_vegetation.py:make_pair (its forcing and initial state, same seed) against
    VegetationOracle(dtype=longdouble, model=dtype): 777 columns, 30 steps of 1800 s.  Compared: PROG + AUX of that module.

    WHERE IT IS MEASURED.  The reference applies its per-year carbon turnover rates per second (tests/workloads.py), so at 1800 s
    the vegetation carbon changes sign and grows by a factor of about 130 every step: 6e64 after 30 steps in fp64.  After an odd
    number of steps the leaf area is hugely negative and exp(-k LAI) of the conductance overflows in the model's format (not in
    long double's); and the fp32 MODEL overflows altogether on the way -- every column is inf or NaN from step 19 on, in the fp32
    oracle as on the device, while the wide instance stays finite, and nothing can be measured there.  The fields are therefore
    compared after `measured` steps: the last step of the 30 at which every compared field of the SAME-PRECISION ORACLE is finite
    in every column (30 in fp64; 16 in fp32 with Euler, 9 with Heun; the reference side alone decides).  After all 30 steps the tested values must be finite exactly where the
    same-precision oracle's are (`final`)."""
    n, nsteps, dt, seed = 777, 30, 1800.0, 1

    def __init__(self, dtype, heun):
        self.dtype, self.heun = np.dtype(dtype), heun
        self.measured, self.final = None, None

    @property
    def id(self):
        return f"vegetation-{self.dtype.name}-{self.n}-{'heun' if self.heun else 'euler'}"

    def inputs(self):
        """(forcing, carbon_vegetation, vegetation_area_fraction) as make_pair draws them"""
        from test_gpu_vegetation import forcing
        rng = np.random.default_rng(self.seed)
        f = forcing(self.n, rng)
        return f, rng.uniform(0.2, 25.0, self.n), rng.uniform(0.0, 0.9, self.n)

    def workload(self):
        return None

    def references(self, w=None):
        from test_gpu_vegetation import AUX, PROG
        names = list(PROG + AUX)
        f, C0, nu0 = self.inputs()
        out = []
        for wide in (False, True):
            o = oracle.VegetationOracle(self.n, dtype=np.longdouble if wide else self.dtype, model=self.dtype)
            for k, v in f.items():
                o.set(k, np.asarray(v, dtype=self.dtype))
            o.set("carbon_vegetation", np.asarray(C0, dtype=self.dtype))
            o.set("vegetation_area_fraction", np.asarray(nu0, dtype=self.dtype))
            snaps = []
            for _ in range(self.nsteps):
                o.timestep(self.dt, True, self.heun)
                snaps.append(fields_of(o, names))
            if not wide:
                finite = [all(np.all(np.isfinite(v)) for v in q.values()) for q in snaps]
                assert any(finite), self.id
                self.measured = max(n + 1 for n in range(self.nsteps) if finite[n])
                self.final = snaps[-1]
            out.append(snaps[self.measured - 1])
        return out[0], out[1], names, None


VEG_STANDALONE = [VegetationCase(nf, heun) for nf in (f64, f32) for heun in (False, True)]

CASES = FP32_PARITY + FP32_DEEP + FP32_C5 + FP64_TOL + FP64_N145 + EXPONENTS + VEG_COUPLED + VEG_STANDALONE
