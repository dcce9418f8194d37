"""The product's HIP sources on the HIP-on-CPU execution model of tests/hipcpu (this container has no GPU).

`warpx_amd/csrc/*.hip` are compiled **unmodified** by the host compiler against a stand-in <hip/hip_runtime.h>
that runs a launch workgroup by workgroup, the work-items as fibers switched at __syncthreads() and at the
wave collectives (64-lane wavefronts, partial exec masks, LDS as per-workgroup storage, atomics).  The
`-m gpu` kernel tests then run against that library exactly as they run against libwarpx_amd.so on the
MI355X: same C-ABI calls, same oracle, same tolerances.  What this checks: indexing, launch geometry, barrier
placement, the logic of the wave-level code and of the LDS-tile kernels.  What it cannot check: anything the
gfx950 compiler or the hardware does differently (FMA contraction, atomics ordering, LDS capacity, timing).

Kept to the kernel-level tests (seconds); the step-level and multi-brick tests run the same way by hand:

    WXA_HIP_ON_CPU=1 python -m pytest tests/test_step_gpu.py tests/test_multibrick_gpu.py -m gpu
"""
import os
import subprocess

import pytest
import sys
from tests.ports import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, extra_env=None, timeout=900):
    env = dict(os.environ, WXA_HIP_ON_CPU="1", **(extra_env or {}))
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-30:])
    assert r.returncode == 0, tail
    return r.stdout


def test_kernel_parity_tests_pass_on_the_cpu_execution_model():
    """Every test of tests/test_kernels_gpu.py, including those still gated on the GPU because no MI355X has
    run them yet (WXA_UNVERIFIED_GPU_TESTS), the geometry sweep of tests/test_geometry_gpu.py (374 cases) and the pushers
    against their model in tests/test_pushers_gpu.py (96 cases)."""
    out = _run(["tests/test_kernels_gpu.py", "tests/test_geometry_gpu.py", "tests/test_pushers_gpu.py"],
               {"WXA_UNVERIFIED_GPU_TESTS": "1"})
    summary = out.strip().splitlines()[-1]
    assert " passed" in summary and "failed" not in summary, summary
    assert int(summary.split(" passed")[0].split()[-1]) >= 110 + 374 + 96, summary


def test_kernel_tests_with_guard_pages_and_fma_contraction():
    """The same tests on the build that contracts a*b+c like hipcc does for device code, every "device" buffer
    (the tests' and the library's) ending on an inaccessible page: no kernel touches memory outside the arrays it
    is handed, and no comparison with the oracle relies on unfused arithmetic.  With tests/test_geometry_gpu.py: this is
    where a staging loop that steps outside a small or offset box faults.  With tests/test_pushers_gpu.py: the pushers'
    gates pay for contraction, and the stragglers there sit in the guard cells."""
    _run(["tests/test_kernels_gpu.py", "tests/test_geometry_gpu.py", "tests/test_pushers_gpu.py"],
         {"HIPCPU_GUARD_PAGES": "1", "WXA_HIP_ON_CPU_FMA": "1"})


def test_short_step_parity_on_the_cpu_execution_model():
    """The whole product schedule (host layer + HIP kernels) against the oracle stepper: order 1 and 3."""
    _run(["tests/test_step_gpu.py", "-k", "test_uniform_plasma_parity or test_reduced_diags_on_the_device"])


def test_output_side_on_the_cpu_execution_model():
    """The tests of the output side that no MI355X has run yet: one plotfile and the reduced-diagnostics rows for all
    bricks of a run (bricks as threads, HIP kernels), and a deck's Full + reduced diagnostics on the HIP path."""
    _run(["tests/test_multibrick_gpu.py", "tests/test_step_gpu.py", "-k",
          "test_one_plotfile_and_reduced_diags_for_all_bricks or test_full_diagnostics_of_a_deck_on_the_hip_path"])


def test_gpu_only_modules_bind_every_global_they_read():
    """The modules only a GPU box executes (tests marked gpu, bench.py, smoke) are otherwise first run at the end
    of a round; a scope-aware pass over their symbol tables catches the NameError class of failure here."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "undefined_names.py")], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout


def test_smoke_body_on_the_cpu_execution_model():
    """__graft_entry__.smoke() minus the device selection."""
    code = ("import __graft_entry__ as g; from tests.oracle_lib import load_hip_on_cpu; "
            "g._smoke(load_hip_on_cpu())")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "[smoke] HIP vs oracle" in r.stdout, (r.stdout + r.stderr)[-2000:]


@pytest.mark.parametrize("nb,port", [((1, 1, 2), 29641), ((1, 2, 2), 29645), ((2, 2, 2), 29646)])
def test_bricks_over_gloo_with_the_hip_kernels(tmp_path, nb, port):
    """The 2-, 4- and 8-GPU layouts of bench.py as separate processes over gloo, every brick running the HIP kernels on the
    execution model with guard-page allocations (a stencil, gather or deposit that leaves a brick's arrays faults):
    separate processes, the real torch.distributed transport, leaver lists, retirement, tile tails."""
    import json
    out = str(tmp_path / "report.json")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "hipcpu"), "-j8"], stdout=subprocess.DEVNULL)
    n = nb[0] * nb[1] * nb[2]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port(port)), os.path.join(ROOT, "tests", "multibrick_worker.py"),
           *[str(v) for v in nb], "3", "1", out, "0"]
    env = dict(os.environ, OMP_NUM_THREADS="1", WXA_WORKER_LIB="hipcpu", HIPCPU_GUARD_PAGES="1", WXA_TEST_STEPS="8")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rep = json.load(open(out))
    assert rep["np_total"] == rep["np_ref"] and rep["inside"] and rep["exchanges"] > 0
    assert all(err < 1e-10 for err in rep["errors"].values()), rep["errors"]
    assert rep["ekin_rel"] < 1e-11 and rep["abs_p_rel"] < 1e-11


def test_boosted_wakefield_deck_on_bricks_with_the_hip_kernels(tmp_path):
    """BASELINE config 5 in small (tests/decks/laser_wakefield_boosted_3d.inputs, first 40 steps) on two bricks over gloo,
    every brick running the product's .hip sources on the execution model: device-side boosted injection per brick, the
    antenna split over the bricks, CKC next to the PEC walls, the windowed sort, the moving window -- against one brick on
    the CPU kernels at the reference's 1e-9.  (Since round 5 the guard points behind a wall and beyond a DOMAIN face are
    left to the next PEC pass as the reference leaves them; behind a wall and beyond a face between two bricks they still
    travel with the exchange, and the charge in the guard columns there is still folded: two layouts, one result.)"""
    import json
    from tests.oracle_lib import load_host_cpu
    from tests.test_inputs_cpu import compare_with_golden
    from warpx_amd.sim import WarpXSim
    deck = str(tmp_path / "inputs")
    text = open(os.path.join(ROOT, "tests", "decks", "laser_wakefield_boosted_3d.inputs")).read()
    open(deck, "w").write(text.replace("max_step = 120", "max_step = 40"))
    one = WarpXSim.from_inputs(load_host_cpu(), deck)
    one.evolve(one.max_step)
    want = one.checksum()
    one.close()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "hipcpu"), "-j8"], stdout=subprocess.DEVNULL)
    out = str(tmp_path / "sum.json")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port(29664)), os.path.join(ROOT, "tests", "deck_worker.py"), "2", "1", "1", deck, out]
    env = dict(os.environ, OMP_NUM_THREADS="1", WXA_WORKER_LIB="hipcpu", WXA_HIP_ON_CPU="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = json.load(open(out))
    assert got["lev=0"]["part_per_cell"] == want["lev=0"]["part_per_cell"]
    compare_with_golden(got, want, 1e-9)


@pytest.mark.parametrize("n,port", [(2, 29661), (4, 29662), (8, 29663)])
def test_bench_control_flow_on_several_ranks(n, port):
    """bench.py --gpus N as the driver launches it (torch.distributed.run, one rank per GPU), on the CPU execution
    model over gloo: brick layout, per-rank particles, the barrier / max-over-ranks timing, the exchange statistics
    and the JSON line of rank 0.  Control flow only."""
    import json
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port(port)), os.path.join(ROOT, "scripts", "bench_on_cpu.py"), "--gpus", str(n),
           "--ncell", "16", "--steps", "3", "--warmup", "1", "--preroll", "2", "--full", "--no-cpu-baseline", "--n1-ms", "1.0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == n and line["scaling"] == "weak" and line["steps"] == 3
    assert line["config"]["bricks"] == {2: [1, 1, 2], 4: [1, 2, 2], 8: [2, 2, 2]}[n]
    assert line["config"]["particles_per_gpu"] == 16 ** 3 * 8 and line["exchange"]["exchanges_per_step"] > 0
    assert line["sanity"]["particles_after"] == n * 16 ** 3 * 8 and line["sanity"]["ok"]
    # the line judges itself: the second-stream overlap is on, the efficiency against the N = 1 figure it was handed, the
    # field bytes a step puts on the wire at most (three split directions at N = 8)
    assert line["config"]["overlap_halo"] is True
    ws = line["weak_scaling"]
    assert ws["n1_ms_per_step"] == 1.0 and abs(ws["efficiency"] - 1.0 / line["ms_per_step"]) < 1e-12
    assert line["exchange"]["field_MB_per_step_upper_bound"] > 0


def test_boosted_wakefield_bench_control_flow_on_the_cpu_execution_model():
    """scripts/bench_lwfa_boosted.py (BASELINE config 5 as a one-GPU throughput line: CKC, Vay, NCI corrector, window,
    antenna, continuous injection) through scripts/bench_on_cpu.py on a tiny grid: the window gains particles while the
    front crosses it and the JSON line carries the per-phase table.  Control flow only."""
    import json
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_on_cpu.py"), "--script",
                        os.path.join(ROOT, "scripts", "bench_lwfa_boosted.py"), "--ncell", "16", "16", "64", "--ppc", "1",
                        "--steps", "3", "--fill-steps", "4"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "particle_steps_per_s" and line["value"] > 0 and line["steps"] == 3
    assert line["config"]["particles_after"] > line["config"]["particles_before"] > 0
    assert {"EvolveB", "EvolveE", "GatherAndPush", "CurrentDeposition", "Redistribute"} <= set(line["kernels"])
    assert line["kernels"]["GatherAndPush"]["launches_per_step"] == 2.0   # the electrons and the antenna


def test_bench_control_flow_on_the_cpu_execution_model():
    """bench.py --full, unmodified, through scripts/bench_on_cpu.py (tiny grid): the JSON line carries the contract's keys
    and the per-phase tables.  A dry run of the control flow only -- the numbers mean nothing."""
    import json
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_on_cpu.py"), "--ncell", "16", "--steps", "2",
                        "--warmup", "1", "--preroll", "2", "--full", "--no-cpu-baseline"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "kernels"):
        assert key in line, key
    assert line["roofline"]["bound"] == "hbm" and line["config"]["workload"].startswith("3D uniform_plasma")
    assert {"EvolveB", "EvolveE", "GatherAndPush", "CurrentDeposition"} <= set(line["kernels"])


def test_plain_bench_line_and_its_outputs_on_the_cpu_execution_model(tmp_path):
    """A plain bench.py run (no --full) times exactly --steps steps and prints the headline keys only; --dump-outputs
    writes the state of the last timed step as float64 .npy files, the same sample in two runs of the same arguments."""
    import json
    import numpy as np
    lines, dumps = [], []
    for run in range(2):
        d = tmp_path / f"out{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bench_on_cpu.py"), "--ncell", "16", "--steps", "3",
                            "--warmup", "1", "--preroll", "2", "--dump-outputs", str(d)], cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
        dumps.append(d)
    line = lines[0]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["metric"] == "particle_steps_per_s" and line["unit"] == "particle-steps/s" and line["higher_is_better"]
    assert line["steps"] == 3 and line["dtype"] == "f64" and line["ms_per_step"] > 0
    assert abs(line["value"] - 16 ** 3 * 8 * 1e3 / line["ms_per_step"]) <= 1e-9 * line["value"]
    for key in ("kernels", "roofline", "sanity", "cpu_baseline"):   # behind --full
        assert key not in line, key
    names = sorted(p.name for p in dumps[0].iterdir())
    assert names == sorted(p.name for p in dumps[1].iterdir())
    assert {"Ex.npy", "By.npy", "jz.npy", "Ez_sumsq.npy", "particles.npy"} <= set(names)
    total = 0
    for name in names:
        a, b = np.load(dumps[0] / name), np.load(dumps[1] / name)
        total += (dumps[0] / name).stat().st_size
        assert a.dtype == np.float64 and a.shape == b.shape and np.all(np.isfinite(a)), name
        assert np.allclose(a, b, rtol=1e-9, atol=0.0), name
    assert total <= 64 * 2 ** 20
    assert np.load(dumps[0] / "particles.npy").shape[0] == 7 and np.max(np.abs(np.load(dumps[0] / "jx.npy"))) > 0
