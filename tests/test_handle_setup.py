"""The library and the host emulation set a handle up through one header (parallel-ddp_amd/csrc/handle_setup.hpp): defaults, the ABI's rules, the array table, the
step-size table and the public view of the solver state are the same on both sides -- the CPU suite measures the kernel bodies against an emulation that is configured
like the product.  And pddp_time_kernels, which launches the production sweeps, marks the reference-layout views stale like pddp_iterate does."""
import ctypes as C
import math

import numpy as np
import pytest

import pyddp
from pyddp.binding import PddpState
from backends import hostsim_path, make_solver
from oracle_binding import example_inputs

PDDP_EINVAL = -1


def _libs():
    libs = C.CDLL(pyddp.library_path()), C.CDLL(hostsim_path())
    for lib in libs:
        lib.pddp_last_error.restype = C.c_char_p
    return libs


def _default(lib, plant):
    c = pyddp.PddpConfig()
    C.memset(C.byref(c), 0xA5, C.sizeof(c))                   # every byte has to come from the callee
    assert lib.pddp_default_config(C.byref(c), plant) == 0
    return c


@pytest.mark.parametrize("plant", [1, 2, 3, 4])
def test_default_config_and_sizes_agree(plant):
    lib, sim = _libs()
    a, b = _default(lib, plant), _default(sim, plant)
    assert bytes(a) == bytes(b)
    assert a.plant == plant and a.N > 0 and a.alpha_base > 0
    assert lib.pddp_state_size(plant) == sim.pddp_state_size(plant) == pyddp.PLANT_DIMS[plant][1]
    assert lib.pddp_control_size(plant) == sim.pddp_control_size(plant) == pyddp.PLANT_DIMS[plant][2]


# one broken rule of the ABI each: (plant, overrides)
BROKEN = [
    pytest.param(1, dict(N=48), id="N-not-a-power-of-two"),
    pytest.param(1, dict(N=64, M=3), id="M-not-dividing-N"),
    pytest.param(1, dict(A=65), id="A-65"),
    pytest.param(2, dict(ee_cost=1), id="ee_cost-on-the-cart-pole"),
    pytest.param(4, dict(ee_type=3), id="ee_type-3"),
    pytest.param(4, dict(use_smooth_abs=1), id="smooth-abs-without-ee_cost"),
    pytest.param(1, dict(use_finite_diff=1, integrator=3), id="finite-differences-with-RK3"),
]


@pytest.mark.parametrize("plant,broken", BROKEN)
def test_both_refuse_a_broken_configuration_in_the_same_words(plant, broken):
    """The rule fails before either side touches a device or allocates anything."""
    said = []
    for lib in _libs():
        c = _default(lib, plant)
        for k, v in broken.items():
            setattr(c, k, v)
        h = C.c_void_p()
        assert lib.pddp_create(C.byref(c), C.byref(h)) == PDDP_EINVAL
        said.append(lib.pddp_last_error().decode())
    assert said[0] == said[1] and said[0], said


# ---- on the GPU: the same handle on both sides
SHARED_ARRAYS = ("xs us ds xb ucur dcur P p Pp pp AB H g KT du ApBK Bdu J dmax dJexp alpha xGoal Jout err alphaOut state "
                 "x_old u_old KT_old xTarget costk tshift Jpart dpart parts_fresh").split()
SMALL = {1: dict(N=16, M=2, A=4), 2: dict(N=16, M=2, A=4), 3: dict(N=16, M=2, A=4), 4: dict(N=32, M=4, A=8)}


def _array_bytes(s, name):
    nb = C.c_size_t(0)
    s._chk(s.lib.pddp_array_bytes(s.h, name.encode(), C.byref(nb)))
    return nb.value


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["float", "double"])
@pytest.mark.parametrize("plant", [1, 2, 3, 4])
def test_arrays_step_sizes_and_state_agree_with_the_emulation(plant, dtype):
    kw = dict(SMALL[plant], batch=2, dtype=dtype)
    sim, hip = make_solver("hostsim", plant, **kw), make_solver("hip", plant, **kw)
    for name in SHARED_ARRAYS:
        assert _array_bytes(sim, name) == _array_bytes(hip, name) > 0, name
    al_sim, al_hip = sim.get("alpha"), hip.get("alpha")
    assert al_sim.tobytes() == al_hip.tobytes()
    np.testing.assert_array_equal(al_hip, np.asarray([math.pow(hip.cfg.alpha_base, float(i)) for i in range(kw["A"])]).astype(hip.dtype))      # alpha_base^i, rounded once
    st = (PddpState * 2)()
    for i in range(2):
        st[i].rho, st[i].drho, st[i].prevJ, st[i].dJ, st[i].z = 12.5 + i, 1.25, 3.7 + i, 0.01, 0.3
        st[i].iter, st[i].alphaIndex, st[i].ignore_defect, st[i].accepted, st[i].done = 3 + i, 2, 1, 1 - i, 0
        st[i].cur, st[i].cur2, st[i].bp_retries, st[i].pw = 1 - i, i, 2, 1 - i
    back = []
    for s in (sim, hip):
        s.set_state(st)
        back.append(s.get_state())
    assert bytes(back[0]) == bytes(back[1])
    for i in range(2):                                        # ... and it is the state that went in, in the handle's element type
        assert back[1][i].prevJ == float(hip.dtype.type(3.7 + i)) and back[1][i].rho == 12.5 + i
        assert (back[1][i].iter, back[1][i].accepted, back[1][i].cur, back[1][i].cur2, back[1][i].bp_retries, back[1][i].pw) == (3 + i, 1 - i, 1 - i, i, 2, 1 - i)
    sim.close(); hip.close()


FUSED = [
    pytest.param(4, dict(batch=1, N=32, M=4, A=8, wafr_urdf=1, total_time=0.5), None, id="arm"),
    pytest.param(3, dict(batch=2, N=16, M=2, A=16, total_time=0.5), dict(cf_bp="mq", cf_fp="cf"), id="quadrotor"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("plant,kw,kernels", FUSED)
def test_time_kernels_marks_the_sweep_operands_stale(plant, kw, kernels):
    """Fused handles compose the sweep maps in the backward pass and do not write A - B K / B du; pddp_get_array rebuilds them when sweeps ran since.  The sweeps of
    pddp_time_kernels count: what it leaves in "ApBK" is what pddp_refresh_reference_views computes, not the array of the sweep before."""
    B, N, n = kw["batch"], kw["N"], pyddp.PLANT_DIMS[plant][1]
    rng = np.random.default_rng(3)
    probs = [example_inputs(plant, N, np.float32, noise=rng.normal(0, 0.002, (N, n))) for _ in range(B)]
    x0, u0, xg = (np.concatenate([p[i] for p in probs]) for i in range(3))
    s = make_solver("hip", plant, dtype=0, tol_cost=0.0, max_iter=10, kernels=kernels, **kw)
    s.load(x0, u0, xg)
    s.iterate(2); s.sync()
    assert not any(st.done for st in s.get_state())
    a = s.get("ApBK")
    names = [nm for nm, _ in s.time_kernels(1)]
    b = s.get("ApBK")
    s.refresh_reference_views()
    c = s.get("ApBK")
    s.close()
    if plant == 4:
        assert "k_bp_mfma" in names and not {"k_sweep_lg", "k_sweep_st", "k_sweep_wg"} & set(names), names
    else:
        assert "k_bp_mq" in names and "k_sweep_maps" in names, names
    assert np.isfinite(c).all()
    assert b.tobytes() == c.tobytes()
    assert a.tobytes() != c.tobytes()
