"""The FEM parameter sets the parameter tests share (tests/test_oracle_fem.py, tests/test_fem_params_gpu.py and the `params` round of
tests/golden/make_fem_golden.py).  `default` is the operating point of Deformable.cpp that every other parity test runs at; the
others make live the terms that point multiplies by zero or by a constant:

  soft_damped   c_M > 0 (the g_m m qdot term and the s_m scale of every assembly kernel), rho != 1000
  near_incomp   nu = 0.49: lambda / mu = 33, the least well conditioned fp32-stored matrix
  auxetic       nu < 0: lambda < 0; c_K = 0
  stiff_long    K-dominated, long solves
  tiny_step     M-dominated: h = 1e-4 and c_K = 0 put Keff near M, Jacobi-PCG ends in fewer than 30 iterations (before the persistent
                solver's first exact-residual refresh) -- the tests assert that regime, it is not taken for granted

Newmark (beta, gamma): the control (1/4, 1/2) makes a6 = (1 - gamma / 2 beta) h = 0, a3 = 1, a5 = -1; the other pairs keep gamma != 2 beta.
"""
import numpy as np

PARAMS = {
    "default":     dict(E=1e7,   nu=0.46,  rho=1000.0, h=0.0333, cM=0.0,  cK=0.01),
    "soft_damped": dict(E=2.5e5, nu=0.30,  rho=1200.0, h=0.01,   cM=0.4,  cK=0.003),
    "near_incomp": dict(E=5e6,   nu=0.49,  rho=1000.0, h=0.0333, cM=0.05, cK=0.02),
    "auxetic":     dict(E=1e6,   nu=-0.3,  rho=800.0,  h=0.02,   cM=0.2,  cK=0.0),
    "stiff_long":  dict(E=5e7,   nu=0.20,  rho=1000.0, h=0.1,    cM=0.0,  cK=0.05),
    "tiny_step":   dict(E=1e7,   nu=0.46,  rho=1000.0, h=1e-4,   cM=1.0,  cK=0.0),
}
NAMES = list(PARAMS)

NEWMARK = [(0.25, 0.5), (0.3025, 0.6), (0.4, 0.6)]

# the persistent solver refreshes its residual from b - A x first at iteration 30 (CGSolver.cpp:129-190 restated); tiny_step stays below
FIRST_REFRESH = 30


def lame(name):
    p = PARAMS[name]
    E, nu = p["E"], p["nu"]
    return nu * E / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu))


def material(name):
    """OrcFem / RefFem keyword arguments"""
    p = PARAMS[name]
    return dict(E=p["E"], nu=p["nu"], rho=p["rho"])


def integrator(name):
    """OrcFem.integrator / RefFem.integrator keyword arguments"""
    p = PARAMS[name]
    return dict(timestep=p["h"], cM=p["cM"], cK=p["cK"])


def handle(name):
    """FemIntegrator keyword arguments"""
    p = PARAMS[name]
    return dict(E=p["E"], nu=p["nu"], rho=p["rho"], timestep=p["h"], damping_mass=p["cM"], damping_stiffness=p["cK"])


def load(name, r):
    """a y load per DOF that moves the body by a comparable amount at every set (scaled with E): -10 per DOF at E = 1e7"""
    f = np.zeros(r)
    f[1::3] = -10.0 * PARAMS[name]["E"] / 1e7
    return f


def live_state(r, fixed, seed=7, q_scale=0.005, v_scale=0.1):
    """a random non-zero (q, qdot), zero on the clamped DOFs: the qdot terms of the right-hand side are live"""
    rng = np.random.default_rng(seed)
    q, qv = rng.normal(size=r) * q_scale, rng.normal(size=r) * v_scale
    q[fixed] = 0
    qv[fixed] = 0
    return q, qv
