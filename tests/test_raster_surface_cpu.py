"""The surface of gags_amd.rasterization after its split into raster_* modules: the names callers, tests and tools import
from it are there; none of the tunables is (they live on raster_tunables alone, so that an assignment on the old module raises
instead of quietly doing nothing); no module binds a tunable by value; and the measurement tools patch attributes that exist."""
import glob
import importlib
import os
import py_compile
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE = ("rasterization", "RasterContext", "default_context", "grad_written", "tile_binning", "Binning",
           "_Project", "_ProjectRaw", "_SH", "_Rasterize",
           "_route", "_Route", "_fwd_flags", "_bwd_flags", "_geom_flags", "_stage_bits",
           "_check_isects", "_check_absgrad_route", "_KeptGrad", "_EarlyRowmap")
# tool -> (module, attribute) it assigns to or calls
TOOL_TARGETS = {
    "block_hist.py": [("raster_function", "_backward_staged")],
    "slot_support.py": [("raster_function", "_backward_staged")],
    "extent_stats.py": [("raster_function", "_backward_staged"), ("rasterization", "tile_binning")],
    "chunk_stats.py": [("raster_function", "_backward_staged"), ("raster_staged", "_rowmap")],
    "row_mask_stats.py": [("raster_function", "_backward_staged"), ("raster_staged", "_rowmap")],
    "trim_breakeven.py": [("rasterization", "RasterContext")],
    "union_rows.py": [("rasterization", "default_context")],
}


def _tunables():
    from gags_amd import raster_tunables as T
    return [name for name in vars(T) if name.isupper() and not name.startswith("_")]


def test_rasterization_exposes_its_surface():
    from gags_amd import rasterization as R
    missing = [name for name in SURFACE if not hasattr(R, name)]
    assert not missing, missing


def test_rasterization_re_exports_no_tunable():
    from gags_amd import rasterization as R
    names = _tunables()
    assert {"TILE", "MAX_ISECTS", "CAP_MARGIN", "ABSGRAD_VALU_MAX_D", "PROW_MAX_BYTES", "EARLY_COUNT", "GEOM_COMPACT_ROWS",
            "ZERO_FILL_MIN_ELEMS", "KEEP_GRAD_SHAPES", "TRIM_LISTS", "KEEP_GRAD", "EARLY_ROWMAP", "CAPACITY_MODE"} <= set(names)
    leaked = [name for name in names if hasattr(R, name)]
    assert not leaked, leaked


def test_no_module_binds_a_tunable_by_value():
    files = sorted(glob.glob(os.path.join(ROOT, "gags_amd", "raster_*.py"))) + [os.path.join(ROOT, "gags_amd", "rasterization.py")]
    assert len(files) >= 8
    by_value = re.compile(r"from\s+(\.|gags_amd\.)raster_tunables\s+import")
    for path in files:
        with open(path) as f:
            assert not by_value.search(f.read()), path
    with open(os.path.join(ROOT, "gags_amd", "raster_tunables.py")) as f:
        assert not re.search(r"^\s*(from\s+\.|from\s+gags_amd|import\s+gags_amd)", f.read(), re.M)  # imports nothing from the package


def test_tools_compile_and_patch_what_exists(tmp_path):
    for tool, targets in TOOL_TARGETS.items():
        path = os.path.join(ROOT, "tools", tool)
        py_compile.compile(path, cfile=str(tmp_path / (tool + "c")), doraise=True)
        with open(path) as f:
            src = f.read()
        for module, attr in targets:
            assert hasattr(importlib.import_module("gags_amd." + module), attr), (tool, module, attr)
            assert module in src and attr in src, (tool, module, attr)
