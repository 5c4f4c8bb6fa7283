"""The rasterizer's module-level constants and environment switches, in one place.  Every raster_* module and
rasterization.py read them as `T.NAME` at call time (`from . import raster_tunables as T`), never by `from ... import NAME`:
one assignment on this module (a test's monkeypatch.setattr, a tool) reaches every reader.  Imports nothing from the package."""
import os

TILE = 16
MAX_ISECTS = 1 << 28  # GAGS_MAX_ISECTS of the C ABI (include/gags_raster.h: 32-bit offsets into the slot tables)
ZERO_FILL_MIN_ELEMS = 1 << 24  # (below that the second stream's hand-over costs more than the zeros)
GEOM_COMPACT_ROWS = True   # gags_raster_bwd_geom: per-slot rows numbered compactly (one prefix sum + a 4-byte readback)
CAP_MARGIN = 1.05
# Channel ranges of the range-staged backward of a by-view multi-GPU step (RasterContext.grad_range_channels): an int (uniform
# ranges) or a tuple of widths (multiples of 128) applied in order, the last one repeated / cut to cover D.
GRAD_RANGE_CHANNELS = 128
# Channels per launch of the rows kernel under the range-staged backward (whole ranges; see _backward_staged).  256 costs 0.15-
# 0.3 ms less on ONE GPU (the weight tiles travel from HBM twice instead of four times) but delivers the first range 0.6 ms
# later; with ~1 ms of xGMI time per 128-channel range the exchange, not the GPU, paces the step at N = 8, and it is kept busy
# earliest by one launch per range (DESIGN.md section 6 has the arithmetic; bench.py reports both).
GRAD_ROWS_GROUP = 128
PROW_MAX_BYTES = 24 << 30  # staged backward: partial rows beyond this are produced per 128-channel range (see _backward_staged)
# List trimming (RasterContext.trim_lists; _trim_lists): None = automatic, for views whose forward scratch would exceed
# TRIM_AUTO_BYTES; True / False force it on / off (GAGS_TRIM_LISTS=1 / 0)
TRIM_LISTS = {"1": True, "0": False}.get(os.environ.get("GAGS_TRIM_LISTS", ""), None)
TRIM_AUTO_BYTES = 48 << 30
# Persistent gradient buffer of the colours-only backward (_KeptGrad): default ON
KEEP_GRAD = os.environ.get("GAGS_KEEP_GRAD", "1") != "0"
KEEP_GRAD_MIN_ELEMS = 0   # (every shape: the small test scenes exercise the same path as C3)
KEEP_GRAD_SHAPES = 2      # buffers a context keeps alive at once (least recently used shape is dropped)
# Row map of the colours-only backward at FORWARD time (RasterContext.early_rowmap; _early_rowmap): default ON
EARLY_COUNT = os.environ.get("GAGS_EARLY_COUNT", "1") != "0"  # 0: the intersection count is read back after the prefix sum
EARLY_ROWMAP = os.environ.get("GAGS_EARLY_ROWMAP", "1") != "0"
# Default of RasterContext.capacity_mode (GAGS_CAPACITY_MODE=1; OFF otherwise): see RasterContext.
CAPACITY_MODE = os.environ.get("GAGS_CAPACITY_MODE", "0") == "1"
ABSGRAD_VALU_MAX_D = 32  # gags_raster_bwd_abs: one channel chunk must cover D
