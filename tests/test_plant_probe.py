"""Every plant, integrator and derivative routine of cddp-cpp_amd/csrc/dev_models.hpp, one routine per item (tests/hip/plant_probe_cases.hpp).

The case bodies are compiled twice over the product header: by hipcc for gfx950 (libcddp_hip_probe.so) and by g++ for the host with
the kernels' arithmetic switches (-ffp-contract=off -DCDDP_TRIG_SHARED=1: the plants in the shared sin / cos, a host build no other
test runs).  Cases per plant (24 model structs; LTIModel<2, 1> stands for the LTI template): f (step of the discrete plants), the
step at all four integrators through the three texts of an integrator (Stepper::step(int, ...), Stepper::step(DynCtx, ...),
roll_step<M, INTEG>) with the redo flag, jac, hess where the build has it, the blocked tensor contraction of the eight plants
whose device build has no hess(), the blocked Jacobian next to the full one.

Point sets (tests/plant_probe.py, fixed seeds, 229 items = three wavefronts and a partial one): the regular set (x ~ N(0, 0.7),
u ~ N(0, 1), unit-dominant quaternions, singular coordinates moved into the plant's range) and the edge set (zero, angles within
3 ulp of multiples of pi / 2, zero quaternion / r = 0 / zero mass, magnitudes of 1e6, and per wavefront two lanes with |angle| in
[1e9, 1e12], one NaN lane, one infinite lane, one lane exactly at 1e9 and one just below).

CPU (host build): blocked contraction == numpy contraction of the full tensors and blocked == full Jacobian, bit for bit, both sets;
the three step texts == each other == the integrator formulas of the twin (oracle/twin/cddp_twin.py::discrete_step) applied to the
probe's own f, bit for bit, on every lane whose redo flag is clear (all lanes for the first two texts); redo == "some stage angle
outside the fast range", worked out from the stage states; ids 0-10 against the C++ oracle in shared-trig mode (step, f, Jacobians bit
for bit, Hessians at 1e-10 as tests/test_host_models.py); ids 11-23 against the twins: f against the twin's own expression in mpmath
at 60 digits, bound = 4 x the twin's own float64 error on the same points (TWIN_F_ERR below); every block of jac and hess against
the twin's own derivative at 60 digits (its autodiff expression on second-order Taylor numbers with mpmath components -- Jet in
tests/golden/spacecraft_twin.py --, the exact derivative of its f for the central-difference plants), bound = 4 x the error of the
twin's float64 complex-step / hyper-dual / central-difference value against that on the same points (TWIN_D_ERR below; for central
differences that figure is the truncation error of h = 2e-5), on all 229 points, with the tolerances of
tests/test_spacecraft_plants.py against the twin's float64 values (1e-12 autodiff, 1e-9 finite differences, 1e-10 Hessians) kept as
a ceiling.  The 4 x bounds are taken from the committed figure or the re-measured one, whichever is smaller: the twin's sines and
cosines are the C library's, so its worst error may move by an ulp with the machine, and only downwards is allowed to matter.
GPU: device == host as numbers (dev_probe.same_numbers) for every case on both sets; lanes that can have taken the libm fallback
(any stage entry non-finite or >= 1e9) are held to the host within 1e-13 of the lane's magnitude (2e-9 for central-difference
Jacobians) and to NaN where the host is NaN: semantics only, loose for a small entry on a lane that also carries 1e9 .. 1e12.  The
direct check of the fallback's values -- mpmath's sine and cosine of the lane's angle at 1e-14 -- covers the f of two plants, the
unicycle and the Dubins car, whose f is that sine and cosine times a speed.  The device's blocked tensor terms == the contraction of
the HOST's full tensors, bit for bit.

Measured (host build, regular set; error = max |got - ref| / max(1, |ref|) against mpmath):
  plant          twin float64   product host build
  euler          5.76e-16       5.75e-16
  quaternion     4.77e-16       4.77e-16
  mrp            6.40e-16       6.40e-16
  twobody        1.35e-16       1.35e-16
  landing2d      3.52e-15       3.51e-15
  dubins         1.46e-16       1.45e-16
  dreyfus        1.46e-15       1.45e-15
  acrobot        3.34e-15       3.28e-15
  usv            1.07e-15       1.06e-15
  forklift       1.09e-16       1.08e-16
  quadrotorrate  3.27e-16       3.27e-16
  linearfuel     2.12e-16       2.12e-16
  nonlinear      5.84e-16       7.06e-16
  (bound = 4 x the twin's column; the two columns coincide where the worst point's error comes from operations the twin and the
  plant share -- sines and cosines differ between glibc and the shared routine by design)
Derivatives against the twin's at 60 digits (host build, regular set, all 229 points; twin float64 / product host build per block;
0 = exact; bound = 4 x the twin's figure):
  plant          F_x                   F_u                   F_xx                  F_uu       F_ux
  euler          5.54e-16 / 7.00e-16   6.11e-17 / 6.11e-17   4.78e-16 / 5.26e-16   0 / 0      0 / 0
  quaternion     5.77e-16 / 5.35e-16   6.11e-17 / 6.11e-17   2.48e-17 / 2.48e-17   0 / 0      0 / 0
  mrp            8.21e-16 / 7.07e-16   6.11e-17 / 6.11e-17   2.48e-17 / 2.48e-17   0 / 0      0 / 0
  twobody        8.73e-11 / 8.73e-11   6.55e-12 / 6.55e-12   (no second-order terms)
  landing2d      2.00e-10 / 2.00e-10   2.00e-10 / 2.00e-10   0 / 0                 0 / 0      3.32e-21 / 8.14e-21
  dubins         2.35e-16 / 1.45e-16   0 / 0                 1.45e-16 / 1.45e-16   0 / 0      0 / 0
  dreyfus        0 / 0                 1.70e-16 / 1.08e-16   0 / 0                 1.02e-16 / 1.03e-16   0 / 0
  acrobot        3.41e-15 / 2.95e-15   5.73e-16 / 5.42e-16   4.00e-15 / 3.72e-15   0 / 0      4.19e-16 / 4.19e-16
  usv            1.20e-15 / 3.25e-16   1.87e-18 / 1.87e-18   2.49e-16 / 2.49e-16   0 / 0      0 / 0
  forklift       3.49e-16 / 1.98e-16   0 / 0                 3.01e-16 / 3.01e-16   0 / 0      0 / 0
  quadrotorrate  9.91e-16 / 8.80e-16   1.85e-16 / 1.48e-16   2.45e-15 / 2.63e-15   0 / 0      5.31e-16 / 5.31e-16
  linearfuel     3.89e-10 / 3.89e-10   3.15e-11 / 3.15e-11   0 / 0                 0 / 0      0 / 0
  nonlinear      2.80e-09 / 2.80e-09   6.75e-12 / 6.75e-12   (no second-order terms)
  (two-body, lander, linear-fuel and nonlinear orbit Jacobians are central differences in both: the figure is their truncation error)
Oracle, shared trig (ids 0-10): step x 4, f and Jacobians bit-equal on all 229 points; Hessians on all 229 points of every plant, the
7-joint arm included, worst 2.2e-15 (3-DOF arm: closed form against the oracle's second-order duals), 0 elsewhere.
Reached by every edge set of a plant with a trigonometric argument: 18 of 229 lanes out of the fast range (7 in [1e9, 1e12], 4 at 1e9,
4 NaN, 3 infinite), 4 to 6 per full wavefront, the other lanes in range; cart-pole and unicycle: redo set on 18 lanes (cart-pole RK4:
45, later stages leave the range on the 1e6 lanes) and clear on the rest, set and clear lanes in every wavefront.  On the MI355X the
lanes held to the fallback's semantics deviate from the host by at most 1.3e-3 of their bound.
"""
import numpy as np
import pytest
import mpmath as mp

import plant_probe as P

# worst error of the twin's own float64 f against its expression at 60 digits, regular set (re-measured by the test; bound = 4 x)
TWIN_F_ERR = {"euler": 5.76e-16, "quaternion": 4.77e-16, "mrp": 6.40e-16, "twobody": 1.35e-16, "landing2d": 3.52e-15, "dubins": 1.46e-16, "dreyfus": 1.46e-15, "acrobot": 3.34e-15, "usv": 1.07e-15, "forklift": 1.09e-16, "quadrotorrate": 3.27e-16, "linearfuel": 2.12e-16, "nonlinear": 5.84e-16}

# the same for the twin's own float64 derivatives (complex step / hyper-dual numbers / central differences) against its derivative at 60
# digits, per block F_x, F_u, F_xx, F_uu, F_ux; 0 = the twin is exact there (structural zeros, zero overrides) and so must the plant be
TWIN_D_ERR = {
    "euler": (5.56e-16, 6.13e-17, 4.80e-16, 0.0, 0.0),
    "quaternion": (5.79e-16, 6.13e-17, 2.50e-17, 0.0, 0.0),
    "mrp": (8.23e-16, 6.13e-17, 2.50e-17, 0.0, 0.0),
    "twobody": (8.75e-11, 6.57e-12),
    "landing2d": (2.02e-10, 2.02e-10, 0.0, 0.0, 3.34e-21),
    "dubins": (2.37e-16, 0.0, 1.47e-16, 0.0, 0.0),
    "dreyfus": (0.0, 1.72e-16, 0.0, 1.04e-16, 0.0),
    "acrobot": (3.43e-15, 5.75e-16, 4.02e-15, 0.0, 4.21e-16),
    "usv": (1.22e-15, 1.89e-18, 2.51e-16, 0.0, 0.0),
    "forklift": (3.51e-16, 0.0, 3.03e-16, 0.0, 0.0),
    "quadrotorrate": (9.93e-16, 1.87e-16, 2.47e-15, 0.0, 5.33e-16),
    "linearfuel": (3.91e-10, 3.17e-11, 0.0, 0.0, 0.0),
    "nonlinear": (2.82e-09, 6.77e-12),
}

ORACLE_TAGS = [p.tag for p in P.PLANTS if p.ref == "oracle"]
TWIN_TAGS = [p.tag for p in P.PLANTS if p.ref == "twin"]
FD_JAC = ("twobody", "landing2d", "linearfuel", "nonlinear")     # central-difference Jacobians (h = 2e-5): ceiling 1e-9, the others 1e-12


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return P.host(tmp_path_factory.mktemp("plant_probe"))


def _sets(pl):
    x, u = P.regular_set(pl)
    xe, ue, fam = P.edge_set(pl)
    return (("regular", x, u), ("edge", xe, ue))


def _hess_inputs(pl, x):
    return P.tensor_inputs(pl, x.shape[0])


def _tensor_compared(pl, x, Q):
    """Which entries of the contraction the blocked routine and the full tensors are held to each other in: all of them, but for the
    surface vessel's Q_uu on a lane whose state is not finite.  Usv3Dof's control Hessian is a zero OVERRIDE in the reference
    (usv_3dof.cpp:237-246), which the host hess() restates by overwriting F_uu; the device contracts the autodiff expression's own
    uu block, which is 0 for every finite state (the expression is linear in tau) and 0 * NaN = NaN otherwise.  A non-finite state
    already makes Q_xx and Q_ux NaN in both builds, so no solve can tell the two apart."""
    keep = np.ones(Q.shape, dtype=bool)
    if pl.tag == "usv":
        keep[~np.all(np.isfinite(x), axis=1), pl.nx * pl.nx + pl.nu * pl.nx:] = False
    return keep


# ================================================================================ the table
def test_every_plant_appears_in_every_comparison(H):
    assert len(P.PLANTS) == 24 and sorted(p.id for p in P.PLANTS) == list(range(24))
    for pl in P.PLANTS:
        for case in ("f", "step", "jac"):
            assert P.has_entry(H, "%s_%s" % (case, pl.tag)), (case, pl.tag)
    # second-order terms: hess() in both builds, or host hess() + the blocked contraction; the two finite-difference orbit plants have
    # neither in either build (kHasHess = false, no HessDyn: the reference's own cross Hessian throws for them)
    assert len(P.HESS_BOTH) == 14 and len(P.BLOCKED) == 8 and P.NO_HESS == ["twobody", "nonlinear"]
    assert len(P.HESS_BOTH) + len(P.BLOCKED) + len(P.NO_HESS) == 24
    for tag in P.HESS_BOTH + P.BLOCKED:
        assert P.has_entry(H, "hess_" + tag), tag
    for tag in P.BLOCKED:
        assert P.has_entry(H, "tensor_" + tag), tag
    for tag in P.NO_HESS:
        assert not P.has_entry(H, "hess_" + tag) and not P.has_entry(H, "tensor_" + tag)
    assert P.JAC_BLOCKED == ["euler", "quaternion", "mrp", "forklift", "quadrotorrate"]
    for tag in P.JAC_BLOCKED:
        assert P.has_entry(H, "jacblk_" + tag), tag
    assert len(ORACLE_TAGS) == 11 and len(TWIN_TAGS) == 13


def test_parameters_are_the_problem_builders(api):
    for pl in P.PLANTS:
        if pl.builder is None:
            continue
        p = getattr(api, pl.builder[0])(api.SOLVER_IPDDP, *pl.builder[1])
        assert p.c.model == pl.id and (p.nx, p.nu) == (pl.nx, pl.nu), pl.tag
        got = list(p.c.model_params)
        assert got[:len(pl.params)] == [float(v) for v in pl.params] and not any(got[len(pl.params):]), pl.tag


# ================================================================================ CPU: blocked against full
@pytest.mark.parametrize("tag", P.BLOCKED)
def test_blocked_tensor_terms_equal_the_full_contraction(H, tag):
    pl = P.BY_TAG[tag]
    for name, x, u in _sets(pl):
        w, Q = _hess_inputs(pl, x)
        full = P.split_hess(pl, P.run(H, "hess_" + tag, P.pack(pl, x, u)))
        want = P.contract(pl, full, w, Q)
        got = P.run(H, "tensor_" + tag, P.pack_tensor(pl, x, u, w, Q)).T
        keep = _tensor_compared(pl, x, Q)
        assert P.same_numbers(got[keep], want[keep]), (tag, name, int(np.sum(keep & ~((got == want) | (np.isnan(got) & np.isnan(want))))))
        if name == "edge":
            print("blocked vs full: %-14s bit-equal on both sets; entries not compared (the vessel's Q_uu on non-finite lanes): %d of %d" % (tag, int(np.sum(~keep)), keep.size))
        assert name != "regular" or (np.all(np.isfinite(want)) and np.any(want != Q))


@pytest.mark.parametrize("tag", P.JAC_BLOCKED)
def test_blocked_jacobian_equals_the_full_one(H, tag):
    pl = P.BY_TAG[tag]
    for name, x, u in _sets(pl):
        Y = P.run(H, "jacblk_" + tag, P.pack(pl, x, u))
        nj = Y.shape[0] // 2
        assert P.same_numbers(Y[:nj], Y[nj:]), (tag, name)
        assert name != "regular" or np.all(np.isfinite(Y))
        # Model::jac is the blocked routine (the forklift divides the map's derivative by the timestep on top)
        J = P.run(H, "jac_" + tag, P.pack(pl, x, u))
        if tag != "forklift":
            assert P.same_numbers(J, Y[:nj]), (tag, name)


# ================================================================================ CPU: the three texts of every integrator
def _step_outputs(pl, Y):
    nx = pl.nx
    return Y[:nx].T, Y[nx:2 * nx].T, Y[2 * nx:3 * nx].T, Y[3 * nx] != 0.0


def check_step_texts(lib, ref_lib, pl, name, x, u, integ):
    """The assertions shared by the CPU test (lib = ref_lib = host) and, for the redo flag, the GPU test."""
    a, b, c, redo = _step_outputs(pl, P.run(lib, "step_" + pl.tag, P.pack(pl, x, u, integ=integ)))
    want, stages = P.numpy_step(ref_lib, pl, integ, x, u)
    flags = P.angle_flags(pl, stages, u)
    if pl.tag in P.TRIG_POLICY:
        assert np.array_equal(redo, flags), (pl.tag, name, integ, np.flatnonzero(redo != flags))
    else:
        assert not np.any(redo), (pl.tag, name, integ)     # no policy: the per-call checks stay, the flag is never raised
    return a, b, c, redo, want, stages, flags


@pytest.mark.parametrize("tag", P.TAGS)
def test_three_step_texts_agree_and_equal_the_integrator_formulas(H, tag):
    pl = P.BY_TAG[tag]
    for name, x, u in _sets(pl):
        for integ in range(4):
            a, b, c, redo, want, stages, flags = check_step_texts(H, H, pl, name, x, u, integ)
            assert P.same_numbers(a, b), (tag, name, integ)
            assert P.same_numbers(a, want), (tag, name, integ, np.flatnonzero(~np.all((a == want) | (np.isnan(a) & np.isnan(want)), axis=1)))
            assert P.same_numbers(c[~redo], a[~redo]), (tag, name, integ)
            if name == "regular":
                assert np.all(np.isfinite(a)) and not np.any(redo)
            assert len(stages) == (1 if pl.discrete else (1, 2, 3, 4)[integ])


# ================================================================================ CPU: ids 0-10 against the C++ oracle, shared trig
def _oracle_problem(api, pl, integ):
    if pl.tag == "lti21":
        p = api.Problem(api.SOLVER_IPDDP, api.MODEL_LTI, integ, 2, 1, 8, pl.dt, np.eye(2), np.eye(1), np.eye(2), np.zeros(2), lti_A=P.LTI_A, lti_B=P.LTI_B)
    else:
        p = getattr(api, pl.builder[0])(api.SOLVER_IPDDP, *pl.builder[1])
        p.c.integrator = integ; p.c.dt = pl.dt; p.dt = pl.dt
    return p


@pytest.mark.parametrize("tag", ORACLE_TAGS)
def test_host_build_in_shared_trig_matches_the_oracle(api, oracle_built, H, tag):
    """The shared-trig host arithmetic of the plants against the oracle's independently written plants (oracle/models.hpp) in the same
    elementary functions: what tests/test_host_models.py demands bit for bit in its shared branch is bit for bit here, and the Hessians
    are within its 1e-10, on all 229 points of every plant."""
    pl = P.BY_TAG[tag]
    x, u = P.regular_set(pl)
    B = x.shape[0]
    f = P.run(H, "f_" + tag, P.pack(pl, x, u)).T
    J = P.run(H, "jac_" + tag, P.pack(pl, x, u)).T
    Hs = P.split_hess(pl, P.run(H, "hess_" + tag, P.pack(pl, x, u)))
    worst_h = 0.0
    with api.shared_trig():
        for integ in range(4):
            o = api.Oracle(_oracle_problem(api, pl, integ))
            a = _step_outputs(pl, P.run(H, "step_" + tag, P.pack(pl, x, u, integ=integ)))[0]
            for i in range(B):
                xd, xn, Fx, Fu = o.dynamics(x[i], u[i])
                assert np.array_equal(a[i], xn), (tag, integ, i, np.max(np.abs(a[i] - xn)))
                if integ:
                    continue
                if not pl.discrete:
                    assert np.array_equal(f[i], xd), (tag, i, np.max(np.abs(f[i] - xd)))
                else:
                    assert np.array_equal(f[i], xn), (tag, i)
                assert np.array_equal(J[i, :pl.nx * pl.nx].reshape(pl.nx, pl.nx), Fx) and np.array_equal(J[i, pl.nx * pl.nx:].reshape(pl.nx, pl.nu), Fu), \
                    (tag, i, np.max(np.abs(J[i, :pl.nx * pl.nx].reshape(pl.nx, pl.nx) - Fx)))
                Ho = o.hessians(x[i], u[i])
                assert Ho is not None
                scale = max(1.0, max(np.max(np.abs(c)) for c in Ho))
                for got, ref in zip(Hs, Ho):
                    worst_h = max(worst_h, float(np.max(np.abs(got[i] - ref))) / scale)
                    assert np.max(np.abs(got[i] - ref)) <= 1e-10 * scale, (tag, i)
    print("oracle, shared trig: %-12s step x4 / f / jac bit-equal on %d points; Hessians worst |diff| / scale = %.2e (bound 1e-10)" % (tag, B, worst_h))


# ================================================================================ CPU: ids 11-23 against the twins
@pytest.mark.parametrize("tag", TWIN_TAGS)
def test_values_against_the_twin_in_mpmath(H, tag):
    pl = P.BY_TAG[tag]
    tw = pl.twin(pl.dt)
    x, u = P.regular_set(pl)
    f = P.run(H, "f_" + tag, P.pack(pl, x, u)).T
    e_tw = e_host = 0.0
    for i in range(x.shape[0]):                       # every point of the regular set
        ref = P.twin_f_mp(tw, x[i], u[i])
        e_tw = max(e_tw, P.err_vs_mp(P.twin_f(tw, x[i], u[i]), ref))
        e_host = max(e_host, P.err_vs_mp(f[i], ref))
    print("f vs mpmath: %-14s twin %.2e   host build %.2e   (committed twin figure %.2e, bound 4 x)" % (tag, e_tw, e_host, TWIN_F_ERR[tag]))
    # the bound comes from the committed figure; a twin that does better on the machine at hand (another libm) tightens it
    assert e_host <= 4.0 * min(TWIN_F_ERR[tag], e_tw), (tag, e_host, e_tw, TWIN_F_ERR[tag])


BLOCKS = ("F_x", "F_u", "F_xx", "F_uu", "F_ux")
CEILING = {"F_x": 1e-12, "F_u": 1e-12, "F_xx": 1e-10, "F_uu": 1e-10, "F_ux": 1e-10}     # tests/test_spacecraft_plants.py, tests/test_remaining_plants.py


@pytest.mark.parametrize("tag", TWIN_TAGS)
def test_derivatives_against_the_twin(H, tag):
    """Every block of jac and hess on every point of the regular set against the twin's own derivative at 60 digits (its autodiff
    expression on second-order Taylor numbers of mpmath components; for the central-difference plants the exact derivative of its f,
    so that the figure is the truncation error of h = 2e-5 plus its rounding).  Bound per block = 4 x the twin's own float64 error
    (complex step / hyper-dual numbers / central differences) against that value on the same points, TWIN_D_ERR; a figure of 0 demands
    the exact value (structural zeros, zero overrides).  The bounds of the existing plant tests against the twin's float64 values stay
    as a ceiling."""
    pl = P.BY_TAG[tag]
    tw = pl.twin(pl.dt)
    nx, nu = pl.nx, pl.nu
    x, u = P.regular_set(pl)
    J = P.run(H, "jac_" + tag, P.pack(pl, x, u)).T
    got = [J[:, :nx * nx].reshape(-1, nx, nx), J[:, nx * nx:].reshape(-1, nx, nu)]
    if pl.hess is not None:
        got += list(P.split_hess(pl, P.run(H, "hess_" + tag, P.pack(pl, x, u))))
    nb = len(got)
    e_tw, e_host, e_rel = [0.0] * nb, [0.0] * nb, [0.0] * nb
    for i in range(x.shape[0]):                       # every point of the regular set
        ref = P.twin_derivs_mp(tw, x[i], u[i], pl.hess is not None)
        twin = list(tw.jac(x[i], u[i], 0.0)) + (list(tw.hess(x[i], u[i], 0.0)) if pl.hess is not None else [])
        for k in range(nb):
            e_tw[k] = max(e_tw[k], P.err_vs_pair(twin[k], ref[k]))
            e_host[k] = max(e_host[k], P.err_vs_pair(got[k][i], ref[k]))
            e_rel[k] = max(e_rel[k], P.rel_err(got[k][i], twin[k]))
    fig = TWIN_D_ERR[tag]
    assert len(fig) == nb
    print("derivatives vs mpmath: %-14s %s" % (tag, "   ".join("%s twin %.2e host %.2e (committed %.2e)" % (BLOCKS[k], e_tw[k], e_host[k], fig[k]) for k in range(nb))))
    for k in range(nb):
        # the bound comes from the committed figure; a twin that does better on the machine at hand (another libm) tightens it
        assert e_host[k] <= 4.0 * min(fig[k], e_tw[k]), (tag, BLOCKS[k], e_host[k], e_tw[k], fig[k])
        assert e_rel[k] < (1e-9 if (k < 2 and tag in FD_JAC) else CEILING[BLOCKS[k]]), (tag, BLOCKS[k], e_rel[k])


# ================================================================================ CPU: what the edge sets reach
def test_edge_sets_reach_the_fallback_and_mixed_redo(H):
    total = 0
    for pl in P.PLANTS:
        x, u, fam = P.edge_set(pl)
        lanes = np.arange(x.shape[0])
        has_angle = bool(pl.ax or pl.au)
        out = P.angle_flags(pl, [x], u)
        if has_angle:
            # the ballot fallback: in every full wavefront some lanes are out of range and most are in range
            for w in range(x.shape[0] // 64):
                n = int(np.sum(out[w * 64:(w + 1) * 64]))
                assert 4 <= n <= 8, (pl.tag, w, n)
            total += int(np.sum(out))
        if pl.tag in P.TRIG_POLICY:
            for integ in range(4):
                redo = _step_outputs(pl, P.run(H, "step_" + pl.tag, P.pack(pl, x, u, integ=integ)))[3]
                for w in range((x.shape[0] + 63) // 64):
                    r = redo[w * 64:(w + 1) * 64]
                    assert np.any(r) and not np.all(r), (pl.tag, integ, w)
                print("reach: %-9s %-5s redo set on %d lanes, clear on %d, every wavefront mixed" % (pl.tag, P.INTEGRATORS[integ], int(np.sum(redo)), int(np.sum(~redo))))
        print("reach: %-14s lanes with an out-of-range angle %3d of %d; families %s" % (pl.tag, int(np.sum(out)), x.shape[0],
              {f: int(np.sum(fam == f)) for f in sorted(set(fam))}))
    assert total > 0


# ================================================================================ GPU
FD_JAC_DEVICE = ("manipulator", "twobody", "landing2d", "linearfuel", "nonlinear")    # Model::jac = central differences, h = 2e-5


def _deviation_on_wild(d, h, wild):
    """Lanes that may have taken the libm fallback: worst |device - host| over the lane's magnitude max(1, max |host|), and whether
    the two agree in structure (NaN where the host has NaN, equal infinities)."""
    d, h = d[wild], h[wild]
    if d.size == 0:
        return 0.0, True
    scale = np.maximum(1.0, np.nanmax(np.where(np.isfinite(h), np.abs(h), 0.0), axis=1, initial=0.0))[:, None]
    with np.errstate(all="ignore"):
        same = (d == h) | (np.isnan(d) & np.isnan(h))
        both = np.isfinite(d) & np.isfinite(h)
        dev = np.where(both & ~same, np.abs(d - h) / scale, 0.0)
    return float(np.max(dev)), bool(np.all(same | both))


class _Report:
    """Collects every mismatch of one plant, so that one GPU run shows them all; the test asserts the list is empty.
    Bound on the fallback lanes: the device's libm and glibc agree in sine and cosine to 1e-14 there (the bound of
    tests/test_dev_elem_gpu.py's fallback check).  A plant's row is a sum of products of at most five sines / cosines with
    coefficients of the row's magnitude, some rows a quotient of two such sums: 10 x 1e-14 of the lane's magnitude.  A
    central-difference Jacobian divides two such values by 2 h = 4e-5: 1e-13 / 2e-5.  The bound is relative to the LANE's largest
    magnitude, so it says little about a small entry next to a 1e9 .. 1e12 one: this is a check of semantics (same structure, same
    size), not of the fallback's values -- those are checked directly, against mpmath, for the f of the unicycle and the Dubins car
    only (test_fallback_lanes_hold_the_sine_and_cosine_of_their_angle)."""
    def __init__(self):
        self.bad, self.worst, self.n_wild = [], 0.0, 0

    def compare(self, dev, hst, wild, what, tol=1e-13):
        eq = (dev == hst) | (np.isnan(dev) & np.isnan(hst))
        rows = np.flatnonzero(~np.all(eq, axis=1) & ~wild)
        if rows.size:
            i = rows[0]; e = np.flatnonzero(~eq[i])[0]
            self.bad.append(what + ("in-range lanes differ", rows[:8].tolist(), "lane %d entry %d: device %r host %r" % (i, e, dev[i, e], hst[i, e])))
        w, structure = _deviation_on_wild(dev, hst, wild)
        self.worst = max(self.worst, w / (tol / 1e-13)); self.n_wild += int(np.sum(wild))
        if not structure or w > tol:
            self.bad.append(what + ("fallback lanes", "worst deviation %.3e (bound %.1e)" % (w, tol), "structure equal: %s" % structure))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", P.TAGS)
def test_device_build_equals_host_build(api, H, tag):
    G = P.device()
    pl = P.BY_TAG[tag]
    nx = pl.nx
    R = _Report()
    for name, x, u in _sets(pl):
        wild0 = P.wild_lanes(pl, [x], u)
        cases = ["f", "jac"] + (["hess"] if pl.hess == "both" else []) + (["jacblk"] if pl.jacblk else [])
        for case in cases:
            X = P.pack(pl, x, u)
            R.compare(P.run(G, "%s_%s" % (case, tag), X).T, P.run(H, "%s_%s" % (case, tag), X).T, wild0, (tag, name, case),
                      tol=1e-13 / 2e-5 if (case == "jac" and tag in FD_JAC_DEVICE) else 1e-13)
        for integ in range(4):
            X = P.pack(pl, x, u, integ=integ)
            dev, hst = P.run(G, "step_" + tag, X).T, P.run(H, "step_" + tag, X).T
            _, stages = P.numpy_step(H, pl, integ, x, u)
            wild = P.wild_lanes(pl, stages, u)
            # the redo flag is a decision: equal on every lane.  Where it is set the caller discards roll_step's x_next (the fast
            # routine's quadrant of an out-of-range angle is an overflowing double -> int conversion): not compared.
            if not np.array_equal(dev[:, -1], hst[:, -1]):
                R.bad.append((tag, name, "step", integ, "redo flags differ", np.flatnonzero(dev[:, -1] != hst[:, -1])[:8].tolist()))
            redo = hst[:, -1] != 0.0
            R.compare(dev[:, :2 * nx], hst[:, :2 * nx], wild, (tag, name, "step", integ, "Stepper texts"))
            R.compare(dev[~redo, 2 * nx:], hst[~redo, 2 * nx:], wild[~redo], (tag, name, "step", integ, "roll_step"))
            try:
                check_step_texts(G, H, pl, name, x, u, integ)
            except AssertionError as e:
                R.bad.append((tag, name, "step", integ, "redo reference", str(e)[:300]))
        if name == "regular" and np.any(wild0):
            R.bad.append((tag, "regular set has fallback lanes"))
    print("device == host: %-14s %d lane-cases held to the fallback's semantics, worst deviation there %.2e of the bound" % (tag, R.n_wild, R.worst / 1e-13))
    for b in R.bad:
        print("MISMATCH", b)
    assert not R.bad, R.bad[:4]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ("unicycle", "dubins"))
def test_fallback_lanes_hold_the_sine_and_cosine_of_their_angle(api, H, tag):
    """In a mixed wavefront the out-of-range lanes get the libm's values (1e-14 against mpmath, NaN for a non-finite angle) and the
    in-range lanes keep their fast values (bit-equal to the host: test_device_build_equals_host_build)."""
    G = P.device()
    pl = P.BY_TAG[tag]
    x, u, fam = P.edge_set(pl)
    f = P.run(G, "f_" + tag, P.pack(pl, x, u)).T
    n = 0
    for i in np.flatnonzero(P.out_of_range(x[:, 2])):
        v = u[i, 0] if tag == "unicycle" else 1.3
        if np.isfinite(x[i, 2]):
            a = mp.mpf(float(x[i, 2]))
            assert abs(f[i, 0] - float(v * mp.cos(a))) <= 1e-14 * abs(v) and abs(f[i, 1] - float(v * mp.sin(a))) <= 1e-14 * abs(v), (tag, i, x[i, 2])
        else:
            assert np.isnan(f[i, 0]) and np.isnan(f[i, 1]), (tag, i)
        n += 1
    assert n >= 12
    print("fallback semantics: %s, %d lanes" % (tag, n))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", P.BLOCKED)
def test_device_blocked_tensor_terms_equal_the_hosts_full_contraction(api, H, tag):
    G = P.device()
    pl = P.BY_TAG[tag]
    for name, x, u in _sets(pl):
        w, Q = _hess_inputs(pl, x)
        want = P.contract(pl, P.split_hess(pl, P.run(H, "hess_" + tag, P.pack(pl, x, u))), w, Q)
        got = P.run(G, "tensor_" + tag, P.pack_tensor(pl, x, u, w, Q)).T
        keep = _tensor_compared(pl, x, Q)
        got = np.where(keep, got, 0.0); want = np.where(keep, want, 0.0)
        R = _Report()
        R.compare(got, want, P.wild_lanes(pl, [x], u), (tag, name, "tensor"))
        for b in R.bad:
            print("MISMATCH", b)
        assert not R.bad, R.bad[:4]


@pytest.mark.gpu
def test_device_library_has_every_entry_point(api):
    G = P.device()
    n = 0
    for pl in P.PLANTS:
        names = ["f_", "step_", "jac_"] + (["hess_"] if pl.hess == "both" else []) + (["tensor_"] if pl.hess == "blocked" else []) + (["jacblk_"] if pl.jacblk else [])
        for nm in names:
            assert P.has_entry(G, nm + pl.tag), nm + pl.tag
            n += 1
        if pl.hess == "blocked":
            assert not P.has_entry(G, "hess_" + pl.tag)        # the device build has no hess() for these
    assert n == 3 * 24 + 14 + 8 + 5
