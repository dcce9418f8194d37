"""boundary.field_lo/hi = absorbing_silver_mueller: the inputs reader's word and the refusals at construction (no GPU).
The kernel and the step are in tests/test_silver_mueller_gpu.py."""
import os
import subprocess
import sys

import pytest

from tests.oracle_lib import load_host_cpu
from warpx_amd import _capi
from warpx_amd.sim import WarpXSim

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DECK = os.path.join(HERE, "decks", "silver_mueller_3d.inputs")
SM = 2   # WXA_BOUNDARY_SILVER_MUELLER (include/warpx_amd.h)

MINIMAL = """
max_step = 1
amr.n_cell = 8 8 8
amr.max_level = 0
geometry.dims = 3
geometry.prob_lo = -1.e-6 -1.e-6 -1.e-6
geometry.prob_hi =  1.e-6  1.e-6  1.e-6
"""


def _write(tmp_path, text):
    p = tmp_path / "deck.inputs"
    p.write_text(text)
    return str(p)


def test_the_python_constant_is_the_header_value():
    assert _capi.BOUNDARY_SILVER_MUELLER == SM
    header = open(os.path.join(os.path.dirname(HERE), "include", "warpx_amd.h")).read()
    assert "#define WXA_BOUNDARY_SILVER_MUELLER 2" in header


def test_other_boundaries_are_still_refused_with_the_list_of_words(tmp_path):
    deck = _write(tmp_path, MINIMAL + "boundary.field_lo = pml pml pml\nboundary.field_hi = pml pml pml\n")
    with pytest.raises(_capi.WxaError) as e:
        WarpXSim.from_inputs(load_host_cpu(), deck)
    assert "'pml' is not on this path (periodic, pec, absorbing_silver_mueller)" in str(e.value)


def test_a_backend_without_the_kernel_refuses_the_boundary_by_name():
    """The oracle-backed build of the host layer (tests/host_cpu) leaves Backend::apply_silver_mueller null."""
    lib = load_host_cpu()
    with pytest.raises(_capi.WxaError) as e:
        WarpXSim.from_inputs(lib, DECK)     # the reader accepts the word, the constructor refuses
    assert "absorbing_silver_mueller" in str(e.value)
    with pytest.raises(_capi.WxaError) as e:
        WarpXSim(lib, (8, 8, 8), (0.0,) * 3, (1e-6,) * 3, field_boundary_lo=(0, 0, SM), field_boundary_hi=(0, 0, 1))
    assert "absorbing_silver_mueller" in str(e.value)
    sim = WarpXSim(lib, (8, 8, 8), (0.0,) * 3, (1e-6,) * 3, field_boundary_lo=(0, 0, 1), field_boundary_hi=(0, 0, 1))
    sim.close()                             # the walls it has are untouched


def product_checks(tmp):
    """With the product's sources on the CPU execution model (tests/hipcpu).  Runs in a process of its own: that library
    is loaded with global symbols, which the other libraries of the CPU suite must not meet."""
    from tests.oracle_lib import load_hip_on_cpu
    lib = load_hip_on_cpu()
    box = ((8, 8, 8), (0.0,) * 3, (1e-6,) * 3)
    # the reader knows the word, in any letter case, next to the other two
    for word in ("absorbing_silver_mueller", "Absorbing_Silver_Mueller"):
        deck = os.path.join(tmp, "ok.inputs")
        with open(deck, "w") as f:
            f.write(MINIMAL + f"boundary.field_lo = periodic {word} {word}\nboundary.field_hi = periodic {word} pec\n")
        sim = WarpXSim.from_inputs(lib, deck)
        sim.evolve(1)
        sim.close()
    # algo.maxwell_solver = ckc with the boundary: refused at construction (the reference asserts Yee)
    for make in (lambda: WarpXSim(lib, *box, maxwell_solver=_capi.SOLVER_CKC, field_boundary_lo=(SM, 0, 0),
                                  field_boundary_hi=(SM, 0, 0)),
                 lambda: WarpXSim.from_inputs(lib, DECK, overrides=["algo.maxwell_solver = ckc"])):
        try:
            make()
        except _capi.WxaError as e:
            assert "absorbing_silver_mueller" in str(e) and "Yee" in str(e), str(e)
        else:
            raise AssertionError("ckc with a Silver-Mueller face was accepted")
    WarpXSim(lib, *box, field_boundary_lo=(SM, 0, 0), field_boundary_hi=(SM, 0, 0)).close()   # Yee: accepted
    # a direction is periodic on both sides or on neither; unknown values stay refused
    for lo, hi in (((SM, 0, 0), (0, 0, 0)), ((3, 0, 0), (3, 0, 0))):
        try:
            WarpXSim(lib, *box, field_boundary_lo=lo, field_boundary_hi=hi)
        except _capi.WxaError:
            pass
        else:
            raise AssertionError(f"field boundaries {lo} / {hi} were accepted")
    print("product checks passed")


def test_the_product_reads_the_word_and_refuses_ckc(tmp_path):
    code = f"from tests.test_silver_mueller_cpu import product_checks; product_checks({str(tmp_path)!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, WXA_HIP_ON_CPU="1"))
    assert r.returncode == 0 and "product checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
