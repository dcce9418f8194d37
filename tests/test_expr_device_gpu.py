"""wxa_expr_eval_device: the postfix programs of host/Parser.hpp run by the device (csrc/expr_device.hpp) against
Parser::eval on the host, expression by expression at 256 points.

Arithmetic, comparisons, and / or, if, sqrt, abs, floor, ceil, min, max, fmod, heaviside and integer powers are
correctly rounded or exact operations done once per program step on either side: the bits must agree.  The
transcendental functions come from two libraries (libm, the device's) that each promise a couple of ulp: relative 1e-13
at arguments with |a| <= 10, the gate test_add_plasma uses for the device's log / sin / cos.

Programs beyond the device evaluator's limits (a value stack of 16, 256 operations) are refused where they would be
uploaded, by name and with the measured figure; nothing is launched."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from warpx_amd import _capi
from warpx_amd.sim import WarpXSim

pytestmark = pytest.mark.gpu

N = 256

# bit for bit
EXACT = [
    "x+y", "x-y", "x*y", "x/y", "-x", "+x", "3.5", "a0*x+2*y-x*y/3",
    "-2^2", "2**-1", "x^3", "x**2", "x^-2", "pow(x,4)", "x^16", "y^-16", "-x^2", "2^3^2",
    "x<y", "x>y", "x<=y", "x>=y", "x==y", "x!=y", "x==x", "x!=x",
    "(x<y) and (y<5)", "(x<y) or (y>5)", "x<y and y<5 or x>2", "x and y", "0 or x",
    "sqrt(y)", "sqrt(x*x+y*y)", "abs(x)", "fabs(x)", "floor(x)", "ceil(x)", "floor(2.5*x)", "ceil(-y)",
    "min(x,y)", "max(x,y)", "min(y,x)", "max(y,x)",
    "fmod(x,y)", "fmod(-7.5,2)", "fmod(x,-3)", "fmod(y,0.7)",
    "heaviside(x,0.5)", "heaviside(0,0.5)", "heaviside(x-x,y)", "heaviside(-y,1)",
    "if(x<0,-x,x)", "if(x<0,if(y<5,1,2),if(y<5,3,4))", "if(if(x<0,0,1),y,-y)",
    "if(y>0,x,1/0)", "if(x==0,7,1/x)", "if(y>0,2*x,sqrt(-y))",
    "(x>=1)*(x<3)*(y-1)", "a0*(1+4*(x*x+y*y)/rc2)*(y>=1)",
]
# relative 1e-13
CLOSE = [
    "exp(x)", "log(y)", "log10(y)", "sin(x)", "cos(x)", "tan(x)", "asin(x/10)", "acos(x/10)", "atan(x)",
    "sinh(x)", "cosh(x)", "tanh(x)", "erf(x/4)", "atan2(x,y)", "atan2(y,x)", "pow(y,x)", "y^2.5", "y**0.5", "y^17",
    "pow(y,-2.5)",
]
CONSTANTS = {"a0": 1e-3, "rc2": 40.0}


@pytest.fixture(scope="module")
def points():
    rng = np.random.default_rng(20240)
    x = rng.uniform(-10.0, 10.0, N)
    y = rng.uniform(0.1, 10.0, N)
    # the special arguments: zero, whole numbers (integer powers, floor / ceil at a whole number), a tie of x and y
    x[:8] = [0.0, 1.0, -1.0, 2.0, -3.0, 2.5, -2.5, 10.0]
    y[:8] = [1.0, 1.0, 2.0, 3.0, 4.0, 0.5, 2.5, 10.0]
    return x, y


def device_eval(product, expr, x, y):
    import torch
    vals = torch.from_numpy(np.concatenate([x, y])).to(H.DEVICE)
    out = torch.zeros(N, dtype=torch.float64, device=H.DEVICE)
    product.expr_eval_device(expr.handle, vals.data_ptr(), N, out.data_ptr(), None)
    H.device_sync()
    return np.array(out.cpu().numpy())


def host_eval(expr, x, y):
    return np.array([expr.eval_host(float(a), float(b)) for a, b in zip(x, y)])


def same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64)) or np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("text", EXACT)
def test_exact_operations_give_the_hosts_bits(product, points, text):
    x, y = points
    e = _capi.Expr(product, text, ("x", "y"), CONSTANTS)
    dev, host = device_eval(product, e, x, y), host_eval(e, x, y)
    bad = np.flatnonzero(~((dev == host) | (np.isnan(dev) & np.isnan(host))))
    assert bad.size == 0, (text, x[bad[:4]], y[bad[:4]], dev[bad[:4]], host[bad[:4]])
    e.close()


@pytest.mark.parametrize("text", CLOSE)
def test_transcendental_functions_agree_to_1e13(product, points, text):
    x, y = points
    e = _capi.Expr(product, text, ("x", "y"), CONSTANTS)
    dev, host = device_eval(product, e, x, y), host_eval(e, x, y)
    assert np.all(np.isfinite(host))
    nz = host != 0.0   # where the host gives an exact 0 (log(1), sin(0)) the bound leaves no room: the same 0
    err = np.abs(dev[nz] - host[nz]) / np.abs(host[nz])
    print(f"{text}: max relative difference {err.max():.3e}")
    assert err.max() <= 1e-13 and np.all(dev[~nz] == 0.0), (text, err.max())
    e.close()


def nested(n):
    """x+(x+(...+x)) with n x's: the value stack gets n deep"""
    return "x+(" * (n - 1) + "x" + ")" * (n - 1)


def chain(n):
    """x+x+...+x with n x's: 2 n - 1 operations at depth 2"""
    return "+".join(["x"] * n)


def test_the_limits_themselves_run(product, points):
    """a stack of exactly 16 and a program of exactly 256 operations are inside the limits: same bits as the host"""
    x, y = points
    for text, want in ((nested(16), (31, 16)), ("-(" + chain(128) + ")", (256, 2))):
        e = _capi.Expr(product, text, ("x", "y"), CONSTANTS)
        assert e.info() == want
        assert same_bits(device_eval(product, e, x, y), host_eval(e, x, y))
        e.close()


def small_sim(product):
    sim = WarpXSim(product, (8, 8, 8), (0.0, 0.0, 0.0), (8e-6, 8e-6, 8e-6), nox=1)
    empty = _capi.ParticleView()
    sid = C.c_int32()
    product.sim_add_species(sim._h, -1.602176634e-19, 9.1093837015e-31, C.byref(empty), C.byref(sid))
    return sim, sid.value


def injector():
    inj = _capi.PlasmaInjector()
    for d in range(3):
        inj.ppc[d] = 1
        inj.lo[d], inj.hi[d] = -1e300, 1e300
    return inj


@pytest.mark.parametrize("text,figure", [(nested(17), "depth 17"), (chain(129), "257 operations")])
def test_programs_beyond_the_limits_are_refused_where_they_are_uploaded(product, text, figure):
    e = _capi.Expr(product, text, ("x", "y", "z"))
    sim, sid = small_sim(product)
    inj = injector()
    rc = product._sim_set_injection_profile(sim._h, sid, C.byref(inj), e.handle, None, 0.0, 1e300, 1, 0)
    assert rc == -1   # WXA_ERR_INVALID_ARG
    msg = product._last_error().decode()
    assert figure in msg and "the density expression" in msg, msg
    view = _capi.ParticleView()
    product.sim_get_particles(sim._h, sid, C.byref(view))
    assert view.np == 0   # nothing was added
    # as a momentum: the same refusal, naming the component
    ok = _capi.Expr(product, "0.0*x", ("x", "y", "z"))
    mom = (C.c_void_p * 3)(ok.handle, e.handle, ok.handle)
    rc = product._sim_set_injection_profile(sim._h, sid, C.byref(inj), ok.handle, mom, 0.0, 1e300, 1, 0)
    assert rc == -1 and figure in product._last_error().decode() and "u_y" in product._last_error().decode()
    # and the evaluation entry refuses it too
    rc = product._expr_eval_device(e.handle, None, 0, None, None)
    assert rc == -1 and figure in product._last_error().decode()
    sim.close()


def test_unknown_names_are_refused_at_compile(product):
    h = C.c_void_p()
    names = (C.c_char_p * 1)(b"x")
    rc = product._expr_compile(b"2*x+nope", names, 1, None, None, 0, C.byref(h))
    assert rc == -1 and not h.value
    assert "unknown name 'nope'" in product._last_error().decode()
    rc = product._expr_compile(b"frob(x)", names, 1, None, None, 0, C.byref(h))
    assert rc == -1 and "unknown function 'frob'" in product._last_error().decode()
