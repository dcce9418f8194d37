"""Regenerates tests/golden/plotfile_reference_reader.json: what the reference's own VisMF / FAB reader
(Tools/PostProcessing/read_raw_data.py of a reference checkout, read-only, imported where it lies) returns for the
plotfile this library writes for tests/decks/langmuir_multi_3d.inputs after 4 steps on the CPU build of the host layer.
tests/test_plotfile_cpu.py holds the library's current output against it.

    python tests/golden/make_plotfile_reader_golden.py <reference checkout>
"""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.oracle_lib import load_host_cpu  # noqa: E402
from warpx_amd.sim import WarpXSim  # noqa: E402

ref_root = sys.argv[1]
spec = importlib.util.spec_from_file_location("ref_read_raw_data", os.path.join(ref_root, "Tools/PostProcessing/read_raw_data.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)
if not hasattr(np, "product"):
    np.product = np.prod   # the reference tool predates numpy 2

sim = WarpXSim.from_inputs(load_host_cpu(), os.path.join(HERE, "..", "decks", "langmuir_multi_3d.inputs"))
sim.evolve(4)
with tempfile.TemporaryDirectory() as tmp:
    plt = os.path.join(tmp, "plt")
    sim.write_plotfile(plt)
    sim.close()
    names = open(os.path.join(plt, "Header")).read().split("\n")
    names = names[2:2 + int(names[1])]
    cell_h = os.path.join(plt, "Level_0", "Cell_H")
    boxes, file_names, offsets, header = ref._read_header(cell_h)
    theirs = ref._read_buffer(plt, cell_h, names)
out = {"source": "Tools/PostProcessing/read_raw_data.py of the reference (_read_header, _read_buffer) on the plotfile of "
                 "tests/decks/langmuir_multi_3d.inputs after 4 steps (tests/golden/make_plotfile_reader_golden.py)",
       "header": {"version": header.version, "how": header.how, "ncomp": header.ncomp,
                  "nghost": [int(v) for v in np.atleast_1d(header.nghost)]}, "file_names": list(file_names), "offsets": [int(o) for o in offsets],
       "boxes": [[[int(v) for v in lo], [int(v) for v in hi]] for lo, hi, _ in boxes],
       "fields": {n: {"shape": list(theirs[n].shape), "sum_abs": float(np.sum(np.abs(theirs[n]))),
                      "max_abs": float(np.max(np.abs(theirs[n]))), "sum": float(np.sum(theirs[n]))} for n in names}}
json.dump(out, open(os.path.join(HERE, "plotfile_reference_reader.json"), "w"), indent=1)
print(json.dumps(out)[:400])
