"""`sparseconvnet.SCN` -- the reference's native-extension namespace, re-implemented on the
MI355X C ABI (include/aabr_hip.h).

Function names, argument order and ownership rules are those of the reference's pybind11
module (SparseConvNet/sparseconvnet/SCN/pybind.cpp:11-235; dispatch in
SCN/sparseconvnet_cuda.cpp:281-455): the caller passes an EMPTY output tensor which is
resized and filled here; optional tensors arrive as empty tensors; d_weight / d_bias arrive
pre-zeroed.  What differs by design: all grid state (hash tables, site lists, rule tables)
lives in HBM inside `Metadata_3`, nothing is rebuilt or copied per layer, and every kernel
runs on the current PyTorch HIP stream.
"""
import collections
import ctypes as C
import os
import struct as _struct
import threading as _threading

import torch

import _hip
from _hip import ptr, stream, check

count_macs = os.environ.get("AABR_COUNT_MACS", "1") != "0"  # the reference returns the multiply-add count of every conv; here the count is
                   # a LAZY number: the rule counts stay on the device until somebody reads it


trace = None  # measurement hook: when set to a list, every conv / dW launch appends
              # (kind, n_in, n_out, gather, rows_in, flags, dtype) -- bench.py uses it to find the dominant kernel


class _TotalsRing(object):
    """Device buffer of per-rule-book rule totals (float64).  A rule book writes its total into the next free
    slot with ONE reduction launch when a layer first asks for it; reading values back is one copy of the
    whole buffer.  When the buffer is full it is read back once, kept on the host under its generation
    number, and reused."""
    CAP = 4096

    def __init__(self, device):
        self.buf = torch.zeros(self.CAP, dtype=torch.float64, device=device)
        self.gen, self.n, self.retired, self._snap = 0, 0, {}, None

    def alloc(self):
        if self.n == self.CAP:
            self.retired[self.gen] = self.buf.tolist()
            self.retired.pop(self.gen - 8, None)
            self.gen, self.n, self._snap = self.gen + 1, 0, None
        self.n += 1
        self._snap = None
        return self.gen, self.n - 1

    def value(self, gen, idx):
        if gen == self.gen:
            if self._snap is None:
                self._snap = self.buf[:self.n].tolist()  # the one read-back (host sync) of a fold
            return self._snap[idx]
        return self.retired[gen][idx]


_rings = {}


def _ring(device):
    r = _rings.get(device)
    if r is None:
        r = _rings[device] = _TotalsRing(device)
    return r


class LazyMacs(object):
    """Sum of (rule-total slot, multiplier) terms that behaves like the float the
    reference returns (`sparseconvnet.forward_pass_multiplyAdd_count += ...`,
    submanifoldConvolution.py:85-94) but performs the device->host read only when the value
    is actually looked at -- so counting costs no host synchronisation in the training loop.
    A term references a slot of the per-device totals buffer (never a rule table); a rule book costs
    one small reduction launch however many layers use it, and the pending list is folded into the
    base value (one read-back) once it holds more than 1024 terms."""
    __slots__ = ("terms", "base")

    def __init__(self, terms=(), base=0.0):
        self.terms, self.base = list(terms), float(base)

    def _value(self):
        if self.terms:
            self.base += sum(ring.value(gen, idx) * m for ring, gen, idx, m in self.terms)
            self.terms = []
        return self.base

    def __add__(self, other):
        if isinstance(other, LazyMacs):
            r = LazyMacs(self.terms + other.terms, self.base + other.base)
        else:
            r = LazyMacs(self.terms, self.base + float(other))
        if len(r.terms) > 1024:
            r._value()
        return r

    __radd__ = __add__

    def __iadd__(self, other):  # `counter += macs` in the layer code: amortised O(1), in place
        if isinstance(other, LazyMacs):
            self.terms.extend(other.terms)
            self.base += other.base
        else:
            self.base += float(other)
        if len(self.terms) > 1024:
            self._value()
        return self

    def __float__(self):
        return self._value()

    def __int__(self):
        return int(self._value())

    def __eq__(self, other):
        return self._value() == float(other)

    def __lt__(self, other):
        return self._value() < float(other)

    def __le__(self, other):
        return self._value() <= float(other)

    def __gt__(self, other):
        return self._value() > float(other)

    def __ge__(self, other):
        return self._value() >= float(other)

    def __hash__(self):
        return hash(self._value())

    def __repr__(self):
        return repr(self._value())

    __str__ = __repr__

    def __format__(self, spec):
        return format(self._value(), spec)


def n_rulebook_bits():
    """pybind.cpp:234"""
    return 32


_key_cache = {}


def _key(t):
    """tuple form of a (small, long-lived, CPU) size tensor; memoised per tensor object/version"""
    if not hasattr(t, "tolist"):
        return tuple(int(x) for x in t)
    k = (id(t), t._version)
    v = _key_cache.get(k)
    if v is None or v[0] is not t:
        if len(_key_cache) > 4096:
            _key_cache.clear()
        v = (t, tuple(int(x) for x in t.tolist()))
        _key_cache[k] = v
    return v[1]


# ------------------------------------------------------------------------------------------------
# geometry plan (extension): inside `with geom_plan():` the rule-book builders below do not launch, they append an
# AabrGeomOp record; the list goes to the library in ONE call (aabr_geom_run) at `flush_geom()` / the end of the block.
# Same entry points, same arguments, same order on the same stream -- only the ~10 us of interpreter + ctypes time per
# launch (x ~250 launches per FPN_Net pass) leave the host's critical path.
# ------------------------------------------------------------------------------------------------
_GEOM = _struct.Struct("<ii10i4q8Q")
assert _GEOM.size == 144
G_SUBM, G_TABLES, G_TILE, G_WIDE, G_PAIRS, G_SITES, G_SOFF, G_BK_BUILD, G_BK_SUBM, G_BK_TABLES = \
    1, 2, 3, 4, 5, 7, 8, 9, 10, 11


class _GeomTLS(_threading.local):
    rec = None        # None: launch immediately; else [bytearray, count, keep-alive list] -- per THREAD: a prefetch
                      # thread records the next batch's builders while the training thread runs its own


_gtls = _GeomTLS()
geom_stats = {"plans": 0, "ops": 0}


def _p(t):
    return t.data_ptr() if t is not None else 0


def _geom(kind, i32=(), i64=(), ps=()):
    """record (inside a geom_plan block) or launch (outside) one builder call"""
    i32 = list(i32) + [0] * (10 - len(i32))
    i64 = list(i64) + [0] * (4 - len(i64))
    ps = list(ps) + [0] * (8 - len(ps))
    r = _gtls.rec
    if r is not None:
        r[0] += _GEOM.pack(kind, 0, *i32, *i64, *ps)
        r[1] += 1
        return
    buf = C.create_string_buffer(_GEOM.pack(kind, 0, *i32, *i64, *ps), 144)
    check(_hip.load().aabr_geom_run(buf, 1, stream()))


def flush_geom():
    """hand the records collected so far to the library (call before anything reads what they produce)"""
    r = _gtls.rec
    if r is None or r[1] == 0:
        return
    buf = (C.c_char * len(r[0])).from_buffer(r[0])
    n = r[1]
    geom_stats["plans"] += 1
    geom_stats["ops"] += n
    try:
        check(_hip.load().aabr_geom_run(buf, n, stream()))
    finally:
        del buf
        r[0] = bytearray()
        r[1] = 0
        del r[2][:]


class geom_plan(object):
    def __enter__(self):
        self.outer = _gtls.rec
        if self.outer is None:
            _gtls.rec = [bytearray(), 0, []]
        return self

    def __exit__(self, *exc):
        if self.outer is None:
            try:
                if exc[0] is None:
                    flush_geom()
            finally:
                _gtls.rec = None
        return False


def _keep(*ts):
    """scratch tensors of recorded launches stay alive until the plan has been handed over"""
    if _gtls.rec is not None:
        _gtls.rec[2].extend(ts)


_parked = []          # (event on the consumer stream, tensors) of dead Metadata objects whose geometry was built elsewhere
_park_lock = _threading.Lock()


def _reap_handed_over():
    """drop the parked geometry whose consumer stream has passed its last use"""
    with _park_lock:
        while _parked and _parked[0][0].query():
            _parked.pop(0)


class _Brick(object):
    """brick form of one scale (csrc/brick.hip, csrc/geom.h BrickLevel): ONE allocation = dense directory (one 16-byte
    entry per super-brick of the extent) followed by the occupied bricks; `ext` = the extent (largest coordinate + 1 per
    axis) the directory covers, `dims` = (super-bricks per axis x3, samples)."""
    __slots__ = ("level", "dims", "packed", "nw", "nb_cap", "v_cap", "bcoord", "meta", "ext", "coords_full")

    def __init__(self, ext, nsamples, nb_bound, v_bound, device, meta, alloc=True):
        self.ext = tuple(int(e) for e in ext)
        self.dims = tuple(max((e + 15) // 16, 1) for e in self.ext) + (max(int(nsamples), 1),)
        assert all(d <= 4096 for d in self.dims[:3]) and self.dims[3] <= 65535
        self.packed = self.dims[0] | (self.dims[1] << 16) | (self.dims[2] << 32) | (self.dims[3] << 48)
        self.nw = self.dims[0] * self.dims[1] * self.dims[2] * self.dims[3]
        self.v_cap = max(min(int(v_bound), self.nw * 4096), 1)
        self.nb_cap = max(min(int(nb_bound), self.v_cap, self.nw * 64), 1)
        self.level = torch.empty(4 * (self.nw + self.nb_cap), dtype=torch.int32, device=device) if alloc else None
        self.bcoord = torch.empty((self.nb_cap, 4), dtype=torch.int32, device=device)
        self.coords_full = torch.empty((self.v_cap, 4), dtype=torch.int32, device=device)
        self.meta = meta

    def dims_c(self):
        return _hip.i32xn(self.dims)

    def dir_ptr(self):
        return self.level.data_ptr()

    def bricks_ptr(self):
        return self.level.data_ptr() + 16 * self.nw

    def tensors(self):
        return [self.level, self.bcoord, self.coords_full, self.meta]


def _brick_build(src_coords, vin_bound, vin_count_ptr, size, stride, out_sp, bk, flags=0, scratch=None):
    """record / launch aabr_brick_build of level `bk` from the sites `src_coords` (flags: 1 = buffers already cleared by
    the caller)"""
    lib = _hip.load()
    if scratch is None:
        scratch = torch.empty(int(lib.aabr_brick_scratch_words(bk.nw, bk.nb_cap)) + 2, dtype=torch.int32,
                              device=bk.level.device)
    sp = scratch.data_ptr() + 4 * ((-scratch.data_ptr() // 4) % 2)              # 8-byte aligned status words
    _geom(G_BK_BUILD, tuple(size) + tuple(stride) + tuple(out_sp) + (flags,), (vin_bound, bk.packed, bk.nb_cap, bk.v_cap),
          (_p(src_coords), vin_count_ptr, bk.level.data_ptr(), bk.bcoord.data_ptr(), bk.coords_full.data_ptr(),
           bk.meta.data_ptr(), sp))
    _keep(scratch)
    return scratch


def _brick_arena(bricks, device):
    """ONE zeroed allocation (one fill) for the directory, the bricks and the scan's scratch (csrc/brick.hip's sizes) of every
    `_Brick` in `bricks` (made with alloc=False): gives each its `level`, returns (arena, [scratch slice per brick])"""
    lib = _hip.load()
    spans, words = [], 0
    for bk in bricks:
        lw = 4 * (bk.nw + bk.nb_cap)
        sw = (int(lib.aabr_brick_scratch_words(bk.nw, bk.nb_cap)) + 3) // 4 * 4
        spans.append((words, lw, sw))
        words += lw + sw
    arena = torch.zeros(max(words, 4), dtype=torch.int32, device=device)
    for bk, (o, lw, sw) in zip(bricks, spans):
        bk.level = arena[o:o + lw]
    return arena, [arena[o + lw:o + lw + sw] for o, lw, sw in spans]


class _Grid(object):
    """one scale of the scene: site list + hash table (replaces SparseGrids, Metadata.h:24-34); with
    Metadata_3(site_order="brick") the hash table is replaced by a brick level (`brick`, keys None)"""
    __slots__ = ("coords", "keys", "cap", "V", "sample_off", "brick")

    def __init__(self, coords, keys, cap, V, sample_off=None, brick=None):
        self.coords, self.keys, self.cap, self.V = coords, keys, cap, V
        self.brick = brick
        # host list: first row of sample b (SparseGrid::ctr, Metadata.h:24-33) for b = 0 .. MAX_SAMPLES, or None
        # when the grid was built without the ride-along read
        self.sample_off = sample_off

    def sample_counts(self, nb):
        """sites per sample for samples 0..nb-1 from the offsets read with V, or None"""
        o = self.sample_off
        if o is None or nb + 1 > len(o):
            return None
        return [o[b + 1] - o[b] for b in range(nb)]


# voxel-scatter form (csrc/voxel_scatter.hip): 2 LDS-binned (default), 1 one atomic per point, 0 generic; AABR_SCATTER
# overrides (the A/B of tools/tools_scatter_kernels.py); below SCATTER_MIN_POINTS the generic form's fewer launches win
scatter_variant = int(os.environ.get("AABR_SCATTER", "2"))
SCATTER_MIN_POINTS = int(os.environ.get("AABR_SCATTER_MIN_POINTS", "32768"))
scatter_stats = {"variant0": 0, "variant1": 0, "variant2": 0, "redone": 0, "brick": 0}
# brick-major rows: the voxel scatter straight into the brick grid (csrc/brick.hip aabr_points_prepare / aabr_points_sites:
# no hash table, no first-seen numbering); False (AABR_BRICK_SCATTER=0): the hash scatter above followed by a renumbering
# (Metadata_3._brickify_input, the first round-5 form) -- kept for the A/B and as a second implementation to test against
brick_scatter = os.environ.get("AABR_BRICK_SCATTER", "1") != "0"

# BLInputLayer mode -> mode of the voxel-scatter kernels.  The BL rule book is NOT the flat one's twin: inputLayerRules keeps
# a site's FIRST point in mode 1 and its LAST in mode 2 (.front() / .back(), IOLayersRules.h:100-111; the kernels follow
# that), blRules overwrites in mode 1 (the LAST point wins) and keeps the FIRST in mode 2.  Mode 0 ("unique and all
# present") runs the summing path and is checked (V == B * L).
BL_KERNEL_MODE = {0: 3, 1: 2, 2: 1, 3: 3, 4: 4}


def derived_cap(E):
    """slots of a derived (strided-level) grid that receives at most E keys: 1.5 E rounded up to a power of two --
    worst-case load 2/3, typical 0.15-0.35 (a level keeps a half to a sixth of the sites it is derived from).  Round 3
    used 2 E: every derived grid of a pass was as large as its base grid and was cleared every step."""
    return _hip.next_pow2(max(64, E + (E + 1) // 2))


def _max_outputs(size, stride):
    """output sites one input site can reach under a filter of `size` moved by `stride`"""
    n = 1
    for a, b in zip(size, stride):
        n *= (a + b - 1) // b
    return n


def _derived_level(E, device):
    """buffers of a derived hash level that receives at most E candidate keys, as aabr_convolution_sites and
    aabr_full_convolution_sites (csrc/geometry.hip) take them: (keys, cap, scratch, out_coords) -- `cap` 16-byte
    entries {key, first, val}, a scratch of E + 4 * ceil(max(E, 1) / 256) + 16 words, one site row per candidate key"""
    cap = derived_cap(E)
    nblk = (max(E, 1) + 255) // 256
    keys = torch.empty(2 * cap, dtype=torch.int64, device=device)
    scratch = torch.empty(E + 4 * nblk + 16, dtype=torch.int32, device=device)
    out_coords = torch.empty((max(E, 1), 4), dtype=torch.int32, device=device)
    return keys, cap, scratch, out_coords


def _derived_level_now(sites, gi, fs, st, osz, E):
    """launch at once the library's `sites` builder (aabr_convolution_sites or aabr_full_convolution_sites: same arguments)
    of the hash level of at most E sites that `gi` reaches; (keys, cap, out_coords, meta): the read of meta[0] sizes the level"""
    dev = gi.coords.device
    keys, cap, scratch, out_coords = _derived_level(E, dev)
    meta = torch.empty(_hip.META_WORDS, dtype=torch.int32, device=dev)
    check(sites(ptr(gi.coords), gi.V, _hip.i32x3(fs), _hip.i32x3(st), _hip.i32x3(osz), ptr(keys), cap, ptr(scratch),
                ptr(out_coords), ptr(meta), stream()))
    return keys, cap, out_coords, meta


kMaxSpatial = 65535  # largest spatial size per axis (coordinates <= 65534: csrc/common.h kMaxCoord)
MAX_SAMPLES = 61     # per-sample offsets that ride along with a grid's site-count read (64-word rows)
BRICK_MAX_DIR_WORDS = 1 << 25   # 512 MiB of directory for the input level; above it a scene keeps its hash grids
brick_stats = {"built": 0, "declined": 0}


def _brick_dir_words(extent):
    w = max(extent[3] + 1, 1)
    for e in extent[:3]:
        w *= max((e + 16) // 16, 1)
    return w


_geom_mailboxes = []     # recycled _hip.Mailbox objects of deferred pyramid reads
_BK_MAX_LEVELS = 48  # brick levels of one Metadata (input + strided levels); one read-back row each:
_BK_ROW = 64 + 16    # [V, per-sample offsets .. (64 words) | the level's meta block (16 words)]


class _Gather(object):
    """one gather table [vol, rows] + its compiled streaming forms (built lazily, cached)"""
    __slots__ = ("table", "counts", "vol", "rows", "_blocks", "_blocks256", "_pairs", "_host_counts", "_total")

    def __init__(self, table, counts, vol, rows):
        self.table, self.counts, self.vol, self.rows = table, counts, vol, rows
        self._blocks = self._blocks256 = self._pairs = self._host_counts = self._total = None

    def total_slot(self):
        """(ring, generation, index) of this rule book's rule total on the device"""
        if self._total is None:
            flush_geom()
            ring = _ring(self.table.device)
            gen, idx = ring.alloc()
            torch.sum(self._ensure_counts(), (0,), dtype=torch.float64, out=ring.buf[idx])
            self._total = (ring, gen, idx)
        return self._total

    def _ensure_counts(self):
        if self.counts is None:  # table built without counts (input side of a strided book)
            flush_geom()         # torch reads the table right away
            nb = (self.rows + 255) // 256
            c = (self.table >= 0).to(torch.int32)
            pad = nb * 256 - self.rows
            if pad:
                c = torch.nn.functional.pad(c, (0, pad))
            self.counts = c.view(self.vol, nb, 256).sum(2, dtype=torch.int32).contiguous().view(-1)
        return self.counts

    def blocks(self):
        """tile blocks for aabr_conv_forward"""
        if self._blocks is None:
            lib = _hip.load()
            w = torch.empty(max(lib.aabr_tile_blocks_words(self.rows, self.vol), 1), dtype=torch.int32,
                            device=self.table.device)
            _geom(G_TILE, (self.vol,), (self.rows,), (_p(self.table), _p(w)))
            self._blocks = w
        return self._blocks

    def blocks_wide(self, tile_rows):
        """128- / 256-row tile blocks for aabr_conv_forward_wide (wide layers)"""
        if self._blocks256 is None:
            self._blocks256 = {}
        w = self._blocks256.get(tile_rows)
        if w is None:
            lib = _hip.load()
            w = torch.empty(max(lib.aabr_wide_blocks_words(self.rows, self.vol, tile_rows), 1), dtype=torch.int32,
                            device=self.table.device)
            _geom(G_WIDE, (self.vol, tile_rows), (self.rows,), (_p(self.table), _p(w)))
            self._blocks256[tile_rows] = w
        return w

    def pairs(self):
        """offset-major compacted pairs for aabr_conv_backward_weight"""
        if self._pairs is None:
            lib = _hip.load()
            w = torch.empty(max(lib.aabr_offset_pairs_words(self.rows, self.vol), 1), dtype=torch.int32,
                            device=self.table.device)
            _geom(G_PAIRS, (self.vol,), (self.rows,), (_p(self.table), _p(self._ensure_counts()), _p(w)))
            self._pairs = w
        return self._pairs

    def rule_counts(self):
        """per-offset rule counts (host list); one small D2H read, cached"""
        if self._host_counts is None:
            c = self._ensure_counts()
            flush_geom()
            self._host_counts = c.view(self.vol, -1).sum(1).tolist() if c.numel() else [0] * self.vol
        return self._host_counts

    def max_chunks(self, n_in, n_out):
        """upper bound on the chunks of the weight-gradient pass"""
        cp = _hip.load().aabr_conv_dw_chunk_pairs(self.rows, self.vol, n_in, n_out)
        bound = (self.vol * self.rows + cp - 1) // cp + self.vol
        # the geometric bound sizes a grow-only scratch of bound * n_in * n_out floats (256->256 on a 1.5 M-site
        # book: ~10 GB); past 256 MB read the true per-offset counts once (one small D2H, cached) instead
        if self._host_counts is None and bound * n_in * n_out * 4 > (256 << 20):
            self.rule_counts()
        if self._host_counts is not None:
            return sum((c + cp - 1) // cp for c in self._host_counts)
        return bound


def prefetch_totals(gathers):
    """rule totals of many rule books with ONE launch (LazyMacs slots; `total_slot` otherwise costs one reduction
    launch per rule book at its first use)"""
    todo = [g for g in gathers if g is not None and g._total is None and g.counts is not None and g.rows > 0]
    if not todo:
        return
    flush_geom()
    ring = _ring(todo[0].table.device)
    es = ring.buf.element_size()
    cs, ns, os_ = [], [], []
    for g in todo:
        gen, idx = ring.alloc()
        g._total = (ring, gen, idx)
        cs.append(g.counts.data_ptr())
        ns.append(g.counts.numel())
        os_.append(ring.buf.data_ptr() + idx * es)
    n = len(todo)
    check(_hip.load().aabr_sum_counts((C.c_void_p * n)(*cs), (C.c_int64 * n)(*ns), (C.c_void_p * n)(*os_), n,
                                      stream()))


class _Table(object):
    """rule book: `out` gathers input rows per output row, `inn` gathers output rows per input row
    (for submanifold books `inn` is `out` read with mirrored offsets)"""
    __slots__ = ("out", "inn", "vol", "V_out", "V_in", "flip_ok")

    def __init__(self, out, inn, vol, V_out, V_in, flip_ok=False):
        self.out, self.inn, self.vol = out, inn, vol
        self.V_out, self.V_in, self.flip_ok = V_out, V_in, flip_ok

    def rule_counts(self):
        return self.out.rule_counts()

    def total_rules(self):
        return float(sum(self.rule_counts()))


def _strided_book(gi, go, fs, st, clip):
    """rule book of a Convolution (filter `fs`, stride `st`, output coordinates clipped to `clip`) from level `gi` onto
    level `go`: the two tables and their count arrays, filled by the hash or the brick table builder through `_geom`
    (recorded inside a geom_plan block, launched at once outside)"""
    vol = fs[0] * fs[1] * fs[2]
    dev = gi.coords.device
    t_out = torch.empty((vol, go.V), dtype=torch.int32, device=dev)
    t_in = torch.empty((vol, gi.V), dtype=torch.int32, device=dev)
    counts = torch.empty(vol * ((go.V + 255) // 256), dtype=torch.int32, device=dev)
    counts_in = torch.empty(vol * ((gi.V + 255) // 256), dtype=torch.int32, device=dev)
    if gi.brick is not None:
        _geom(G_BK_TABLES, fs + st + clip, (gi.V, go.V, gi.brick.packed, go.brick.packed),
              (_p(gi.coords), gi.brick.level.data_ptr(), _p(go.coords), go.brick.level.data_ptr(), _p(t_out), _p(t_in),
               _p(counts), _p(counts_in)))
    else:
        _geom(G_TABLES, fs + st + clip, (gi.V, gi.cap, go.V, go.cap),
              (_p(gi.coords), _p(gi.keys), _p(go.coords), _p(go.keys), _p(t_out), _p(t_in), _p(counts), _p(counts_in)))
    return _Table(_Gather(t_out, counts, vol, go.V), _Gather(t_in, counts_in, vol, gi.V), vol, go.V, gi.V)


def _empty_book(vol, device):
    """the rule book between two empty levels: vol x 0 tables, no counts"""
    side = lambda: _Gather(torch.empty((vol, 0), dtype=torch.int32, device=device),
                           torch.empty(0, dtype=torch.int32, device=device), vol, 0)
    return _Table(side(), side(), vol, 0, 0)


def _carve(names, device, unpadded=(), tail=0):
    """ONE int32 allocation carved into the pieces `names` = [(name, words)], in that order: each piece starts where the
    one before it ends rounded up to 16 bytes -- not rounded after a piece named in `unpadded` -- and `tail` words follow
    the last.  Returns (buffer, {name: piece}, {name: offset in words})."""
    offs, tot = {}, 0
    for name, sz in names:
        offs[name] = tot
        tot += sz if name in unpadded else (sz + 3) & ~3
    buf = torch.empty(tot + tail, dtype=torch.int32, device=device)
    return buf, {name: buf[offs[name]:offs[name] + sz] for name, sz in names}, offs


_pinned_pool = []  # (pinned int32[META_WORDS], event) pairs of finished asynchronous read-backs


def _post_meta(meta):
    """enqueue the asynchronous read-back of an input layer's meta block: pinned buffer + event from a small recycling
    pool (allocating pinned memory per scene costs more than the whole enqueue)"""
    host, ev = _pinned_pool.pop() if _pinned_pool else (
        torch.empty(_hip.META_WORDS, dtype=torch.int32, pin_memory=True), torch.cuda.Event())
    host.copy_(meta, non_blocking=True)
    ev.record()
    return host, ev


def _collect_meta(pend):
    """host list of the meta block of a pending input layer: wait for the read-back `_post_meta` enqueued (its buffers
    go back to the pool), or read it now when none was posted"""
    if pend["event"] is None:
        return _hip.read_back(pend["meta"])
    pend["event"].synchronize()
    m = pend["host"].tolist()
    if len(_pinned_pool) < 16:
        _pinned_pool.append((pend["host"], pend["event"]))
    return m


class Metadata_3(object):
    """Replaces Metadata<3> (SCN/Metadata/Metadata.h:44-163, pybind class Metadata_3,
    pybind.cpp:12-32,205).  Caches are keyed exactly like the reference's: grids by spatial
    size, submanifold rule books by (spatial, filter), strided rule books by
    (input spatial, filter, stride) (Metadata.cpp:429-443,484-510)."""

    dimension = 3

    def __init__(self, site_order="first_seen"):
        """`site_order` (extension): "first_seen" = the reference's numbering of the input sites (IOLayersRules.h:86-91,
        exact) over hash grids; "brick" = every level numbered brick by brick (csrc/brick.hip): the same sites, rule
        books and features up to a per-sample permutation of the rows, spatial neighbours adjacent in
        memory, no hash tables -- what FPN_Net(site_order="brick") / bench.py run on."""
        self._handed_over = None    # (consumer stream, tensors) once hand_over() was called: lifetime, not content
        assert site_order in ("first_seen", "brick")
        self.site_order = site_order
        self.input_spatial = None   # spatial size of the input level (setInputSpatialSize / the input layer); survives clear()
        self.clear()

    def clear(self):
        """Metadata::clear (Metadata.cpp:51-65): drop everything derived from an input; the input spatial size stays.
        Every attribute of the object is assigned here or in __init__ -- nothing is created on first use."""
        self.grids = {}                       # spatial size -> _Grid
        self.submanifold = {}                 # spatial + filter -> _Table
        self.rulebooks = {}                   # input spatial + filter + stride -> _Table
        self.fullConvolutionRuleBook = None   # the one rule book of the FullConvolution that created this object
        self._borrowed = set()                # spatial sizes whose level belongs to another Metadata (getFullConvolutionRuleBook)
        self.input = None  # dict(point_site, first_pt, cnt_extra, head, nxt, last_pt, meta, n, V, mode, spatial)
        self.device = None                    # device of the input layer
        self._inb = None                      # incremental input being collected on the host: dict(rows, locs, nsamples)
        # input layer enqueued, not finished; ONE of two shapes: hash scatter dict(host, event, meta, buf, coords, site_coords,
        # keys, cap, variant, redo), brick scatter dict(kind="brick", host, event, meta, buf, coords, piece, spatial_t, mode,
        # device, bl)
        self._pending = None
        self._batch_size_cache = None         # number of samples (SCN._batch_size; a BL input layer knows it at once)
        self._pregrids = set()                # spatial sizes of levels built ahead of the rule book that will claim them
        self._brick_rows = None               # read-back block of the brick levels: one [V, sample offsets | meta] row each
        self._brick_nrows = 0                 # rows of it in use
        self._brick_rows_clean = False        # the unused rows are still zero (allocated zeroed): a pyramid need not fill them
        self._brick_keep = []                 # device tensors of the brick levels that no _Grid holds (arenas, scratch, rows)
        self._pyramid_pending = None          # (todo, made, first_row, posted read) of buildBrickPyramid(defer=True)
        self._fpn_prebuilt = None             # FPN_Net.prebuild: the level sizes whose geometry is already built
        self._defer_pyramid = False           # FPN_Net.prepare: the next pyramid's read is collected later
        self._roi_extent = {}                 # spatial size -> occupied extent (roi_align_rotated_3d._occupied_extent)
        self._roi_cellmap = {}                # spatial size -> cell map tensor (roi_align_rotated_3d._cellmap)

    def _materialised(self):
        """the device grid of an incremental input, if one is still being collected"""
        if self._inb is not None:
            self._materialise_input(torch.device("cuda", torch.cuda.current_device()))

    # ---- reference-visible queries ----------------------------------------------------
    def getSpatialLocations(self, spatial_size):
        """LongTensor [V,4] (x,y,z,batch), CPU like the reference (Metadata.cpp:147-168)."""
        return self.getSpatialLocationsDevice(spatial_size).cpu()

    def getSpatialLocationsDevice(self, spatial_size):
        self._materialised()
        g = self.grids[_key(spatial_size)]
        loc = torch.empty((g.V, 4), dtype=torch.int64, device=g.coords.device)
        check(_hip.load().aabr_spatial_locations(ptr(g.coords), g.V, ptr(loc), stream()))
        return loc

    def hand_over(self, consumer):
        """Geometry built on another stream (FPN_Net.prepare) is about to be used on `consumer`.  Its tensors' memory
        belongs to the producer stream's pool; it must not be reused there before `consumer` has passed every launch
        that reads it.  `tensor.record_stream(consumer)` does that PER TENSOR: at free time the allocator records one
        event on the consumer stream for each of the ~200 geometry tensors of a pass -- 200 marker packets between two
        training steps, measured as 1.07 ms of idle main stream per 14.4 ms step (tools/tools_step_timeline.py,
        profiles/r03_step_timeline.txt).  Instead the tensors are kept until this object dies, then parked with ONE
        event recorded on the consumer stream and dropped when that event has passed (`_reap_handed_over`).
        Everything that enqueues reads of this geometry on `consumer` holds THIS object until it has enqueued them --
        the SparseConvNetTensors of the pass, the compiled `_Pass` (planExecutor: `ps.md`, kept by the autograd node
        until its backward list is out) and every per-layer Function ctx (`ctx.input_metadata`) -- so the parking event
        recorded in __del__ lies behind the last such read."""
        self._handed_over = (consumer, self.device_tensors())

    def __del__(self):
        ho = self._handed_over
        if ho is None:
            return
        try:
            ev = torch.cuda.Event()
            ev.record(ho[0])
            with _park_lock:
                _parked.append((ev, ho[1]))
        except Exception:     # interpreter shutdown: the process's memory goes away with it
            pass

    def device_tensors(self):
        """every device tensor this object owns (for cross-stream hand-over of geometry prepared ahead of time)"""
        ts = []
        if self._pending is not None:
            ts += [self._pending["buf"]]
        for g in self.grids.values():
            ts += [g.coords] + ([g.keys] if g.keys is not None else []) + (g.brick.tensors() if g.brick is not None else [])
        ts += list(self._brick_keep)
        if self.input is not None:
            ts += [self.input["point_site"]]
        full = [self.fullConvolutionRuleBook] if self.fullConvolutionRuleBook is not None else []
        for tb in list(self.submanifold.values()) + list(self.rulebooks.values()) + full:
            for ga in (tb.out, tb.inn):
                if ga is None:
                    continue
                ts += [t for t in (ga.table, ga.counts, ga._blocks, ga._pairs) if t is not None]
                if ga._blocks256:
                    ts += list(ga._blocks256.values())
        return ts

    def getNActive(self, spatial_size):
        if self._inb is not None and _key(spatial_size) == self.input_spatial:
            return len(self._inb["locs"])
        return self.grids[_key(spatial_size)].V

    def setInputSpatialSize(self, spatial_size):
        """Metadata::setInputSpatialSize (Metadata.cpp:76-80)"""
        self.input_spatial = _key(spatial_size)

    # ---- incremental input construction (pybind.cpp:15-19; Metadata.cpp:81-145, 30-44) --------------------------
    # The reference fills the caller's `features` tensor on the HOST, one location at a time: a location not seen
    # before in the sample appends a row (first-seen numbering across all calls), a repeated one overwrites its row
    # or is ignored.  Same here, in Python (this is host bookkeeping in the reference too); the DEVICE grid of the
    # collected sites is built at the first geometry query (`_materialise_input`) through the voxel-scatter kernels.
    def _collecting(self):
        assert self.input_spatial is not None, "Call setInputSpatialSize first, please!"
        if self._inb is None:
            self._inb = dict(rows={}, locs=[], nsamples=0)
        return self._inb

    def batchAddSample(self):
        self._collecting()["nsamples"] += 1

    def _add_point(self, features, key, vec, overwrite, rows_out):
        b = self._inb
        r = b["rows"].get(key)
        if r is None:
            b["rows"][key] = len(b["locs"])
            b["locs"].append(key)
            rows_out.append((len(b["locs"]) - 1, vec))
        elif overwrite:
            rows_out.append((r, vec))

    def _flush_rows(self, features, planes, rows):
        n = len(self._inb["locs"])
        old = features.clone() if features.numel() else None
        features.resize_(n, planes)
        if old is not None:
            features[: old.shape[0]] = old
        for r, vec in rows:
            features[r] = vec

    def setInputSpatialLocation(self, features, location, vec, overwrite):
        assert self._inb and self._inb["nsamples"] > 0, "call batchAddSample first"
        rows = []
        key = (self._inb["nsamples"] - 1,) + tuple(int(v) for v in location.tolist())
        self._add_point(features, key, vec, overwrite, rows)
        self._flush_rows(features, int(vec.shape[0]), rows)

    def setInputSpatialLocations(self, features, locations, vecs, overwrite):
        b = self._collecting()
        L = locations.tolist()
        rows = []
        for i, loc in enumerate(L):
            if len(loc) == self.dimension:
                assert b["nsamples"] > 0, "call batchAddSample first"
                key = (b["nsamples"] - 1,) + tuple(int(v) for v in loc)
            else:                                       # 4th column = sample index; grows the batch as needed
                key = (int(loc[-1]),) + tuple(int(v) for v in loc[:-1])
                b["nsamples"] = max(b["nsamples"], key[0] + 1)
            self._add_point(features, key, vecs[i], overwrite, rows)
        self._flush_rows(features, int(vecs.shape[1]), rows)

    def _materialise_input(self, device):
        """device grid of the incrementally collected sites (unique by construction, sample-major like the
        reference's per-sample grids with their `ctr` offsets)"""
        b, self._inb = self._inb, None
        if b is None or self.input is not None:
            return
        order = sorted(range(len(b["locs"])), key=lambda i: (b["locs"][i][0], i))   # samples contiguous, first-seen inside
        if order != list(range(len(order))):
            raise _hip.AabrError("incremental input: add the samples one after the other (rows of a sample must be "
                                 "contiguous, as Metadata::getSpatialLocations' ctr offsets assume)")
        coords = torch.tensor([list(k[1:]) + [k[0]] for k in b["locs"]], dtype=torch.int64).reshape(-1, 4)
        self.inputLayer(torch.LongTensor(list(self.input_spatial)), coords, b["nsamples"], 3, device)

    # ---- builders ---------------------------------------------------------------------------
    def inputLayer(self, spatial_size, coords, batch_size, mode, device):
        """Metadata::inputLayer (Metadata.cpp:405-417)"""
        return self._input_layer(spatial_size, coords, mode, device, False)

    def blLayer(self, spatial_size, coords, mode, device=None):
        """Metadata::blLayer (Metadata.cpp:419-428 -> blRules, IOLayersRules.h:127-297): the input layer of a padded batch,
        coords int64 [B, L, 3] read where they lie (csrc/point_reader.h BLReader); `mode` is the BL mode 0..4 (BL_KERNEL_MODE
        maps it to the kernels' mode).  Returns V; the object then holds exactly B samples."""
        if device is None:
            device = coords.device if coords.is_cuda else torch.device("cuda", torch.cuda.current_device())
        V = self._input_layer(spatial_size, coords, BL_KERNEL_MODE[int(mode)], device, True)
        self.input["bl_mode"] = int(mode)       # what blLayerRuleBook reports (input["mode"] is the kernels' mode)
        return V

    def _input_layer(self, spatial_size, coords, mode, device, bl):
        if self.input is not None:
            src = self.input.get("coords_src")
            if src is not None and src[0] is coords and src[1] == coords._version and self.input["mode"] == int(mode) \
                    and (self.input.get("bl") is not None) == bl:
                return self.inputLayerFinish()  # prepared ahead of time (InputLayer.prepare / BLInputLayer.prepare)
        self.inputLayerEnqueue(spatial_size, coords, mode, device, asynchronous=False, bl=bl)
        return self.inputLayerFinish()

    def inputLayerEnqueue(self, spatial_size, coords, mode, device, asynchronous=True, bl=False):
        """enqueue the site-numbering kernels (+ an asynchronous read-back of (V, maxActive, err)
        when `asynchronous`); all integer state of the input layer lives in ONE device allocation.
        `bl`: coords is the padded batch [B, L, 3] of a BLInputLayer instead of the flat [n, 3 or 4] list: the same
        kernels read it in place through the BL reader (point i = flat row b * L + l, batch index i / L, x < 0 = empty);
        `mode` is the KERNELS' mode either way."""
        if bl:
            assert coords.dim() == 3 and coords.size(2) == 3
        else:
            assert coords.dim() == 2 and coords.size(1) in (3, 4)
        assert self.input is None and len(self.grids) == 0, "Metadata already holds an input layer"
        coords_src = (coords, coords._version)   # identity + version of the caller's tensor (kept alive here)
        lib = _hip.load()
        self.device = device
        coords = coords.to(device=device, dtype=torch.int64, non_blocking=True).contiguous()
        if bl:
            B, L = int(coords.shape[0]), int(coords.shape[1])
            n, ncols, shape = B * L, 3, (B, L)
            self._batch_size_cache = B          # B samples, empty ones included (the flat form derives it from the sites)
            sites = lambda *a: lib.aabr_bl_input_layer_sites(ptr(coords), B, L, *a)
        else:
            n, ncols = coords.shape
            shape = None
            sites = lambda *a: lib.aabr_input_layer_sites(ptr(coords), n, ncols, *a)
        if self.site_order == "brick" and brick_scatter and n > 0:
            return self._enqueue_brick_scatter(spatial_size, coords, coords_src, mode, device, asynchronous, shape)
        cap = _hip.next_pow2(2 * n)
        n1 = max(n, 1)
        nst = int(lib.aabr_input_layer_status_words(n))
        # Which form of the insert (csrc/voxel_scatter.hip): 2 = LDS-binned, 1 = one atomic per point, 0 = generic (two
        # atomics per point; any coordinates).  The first two need (batch, x, y, z, point index) in one 64-bit word --
        # widths from the layer's spatial size and n -- and are only worth their extra launch from a few 10^4 points on;
        # a point that does not fit is reported through meta[5] and the generic form runs instead (inputLayerFinish).
        sp3 = _hip.i32x3(_key(spatial_size))
        variant = 0 if bl else scatter_variant      # (the packed / LDS-binned inserts read the flat list only)
        if variant and (n < SCATTER_MIN_POINTS or lib.aabr_input_layer_pack_bits(n, sp3) < 2):
            variant = 0
        if variant == 2 and not (4096 <= cap <= (1 << 24)):
            variant = 1
        # int32 words, 16-byte aligned pieces; the grid's 16-byte entries {key, first, val} and meta sit back to back
        # so the library clears them with ONE fill:  grid(4*cap) meta(8) | slot(n) point_site(n) nxt(n)
        #                      site_coords(4*n1) first_pt(n1) cnt_extra(n1) head(n1) last_pt(n1) status(nst)
        names = [("keys", 4 * cap), ("meta", _hip.META_WORDS), ("slot", n),
                 ("point_site", n), ("nxt", n), ("site_coords", 4 * n1), ("first_pt", n1), ("cnt_extra", n1),
                 ("head", n1), ("last_pt", n1), ("status", nst)]
        if variant:      # scratch of the packed forms: cap 8-byte words + one cursor per 4096-slot block
            names += [("words", 2 * cap), ("cursor", max(cap // 4096, 1))]
        buf, piece, offs = _carve(names, device)
        keys = piece["keys"].view(torch.int64)    # cap entries of 16 bytes: {uint64 key, uint32 first, int32 val}
        meta = piece["meta"]
        site_coords = piece["site_coords"].view(n1, 4)
        base = buf.data_ptr()
        P = lambda name: base + 4 * offs[name]
        generic = lambda: check(sites(P("keys"), cap, P("slot"), P("point_site"), P("site_coords"), P("first_pt"),
                                      P("cnt_extra"), P("head"), P("nxt"), P("status"), P("meta"), stream()))
        host = ev = None
        if n > 0:
            if variant:
                check(lib.aabr_input_layer_sites_packed(ptr(coords), n, ncols, sp3, variant, P("keys"), cap, P("words"),
                                                        P("cursor"), P("slot"), P("point_site"), P("site_coords"),
                                                        P("first_pt"), P("cnt_extra"), P("head"), P("nxt"), P("status"),
                                                        P("meta"), stream()))
            else:
                generic()
            if asynchronous:
                host, ev = _post_meta(meta)
        else:  # empty scene: an empty grid (all keys EMPTY), nothing to launch
            keys.fill_(-1)
            meta.zero_()
        self._pending = dict(host=host, event=ev, meta=meta, site_coords=site_coords, keys=keys,
                             cap=cap, coords=coords, buf=buf, variant=variant, redo=generic)
        scatter_stats["variant%d" % variant] += 1
        self._set_input(piece, n, mode, spatial_size, coords_src, shape)

    def _set_input(self, piece, n, mode, spatial_size, coords_src, bl):
        """the input layer's record over the carved pieces of either scatter (`bl`: (B, L) of a padded batch, or None)"""
        self.input = dict(point_site=piece["point_site"], first_pt=piece["first_pt"], cnt_extra=piece["cnt_extra"],
                          head=piece["head"], nxt=piece["nxt"], last_pt=piece["last_pt"], meta=piece["meta"], n=n, V=None,
                          mode=int(mode), spatial=_key(spatial_size), coords_src=coords_src, bl=bl)

    def _enqueue_brick_scatter(self, spatial_size, coords, coords_src, mode, device, asynchronous, bl=None):
        """brick-major rows WITHOUT a hash table (csrc/brick.hip "voxel scatter straight into a brick grid"): the points are
        converted and their extent reduced now (one kernel + the asynchronous read of the extent); `inputLayerFinish` sizes
        the directory by it, builds the input level from the points and hands every point its row"""
        lib = _hip.load()
        if bl is not None:                      # the padded batch [B, L, 3] of a BLInputLayer, converted where it lies
            n = bl[0] * bl[1]
            prepare = lambda *a: lib.aabr_bl_points_prepare(ptr(coords), bl[0], bl[1], *a)
        else:
            n, ncols = coords.shape
            prepare = lambda *a: lib.aabr_points_prepare(ptr(coords), n, ncols, *a)
        names = [("pc", 4 * n), ("meta", _hip.META_WORDS), ("point_site", n), ("nxt", n), ("first_pt", n), ("head", n),
                 ("cnt_extra", n), ("last_pt", n)]
        buf, piece, _ = _carve(names, device, unpadded=("first_pt",), tail=4)   # first_pt | head contiguous: ONE fill for the two
        meta = piece["meta"]
        # (the per-site arrays' starting values ride in this pass: aabr_points_sites(flags = 1) then fills nothing)
        check(prepare(piece["pc"].data_ptr(), meta.data_ptr(), ptr(piece["first_pt"]), ptr(piece["cnt_extra"]),
                      ptr(piece["head"]), stream()))
        host, ev = _post_meta(meta) if asynchronous else (None, None)
        self._pending = dict(kind="brick", host=host, event=ev, meta=meta, coords=coords, buf=buf, piece=piece,
                             spatial_t=spatial_size, mode=mode, device=device, bl=bl)
        scatter_stats["brick"] = scatter_stats.get("brick", 0) + 1
        self._set_input(piece, n, mode, spatial_size, coords_src, bl)

    def _brick_scatter_launch(self, piece, n, key, extent, dev):
        """the launches of the brick-native scatter behind the extent read: input level from the points, then every point's
        row / first point / chain (no host read in here -- bench.py times exactly this)"""
        lib = _hip.load()
        # read-back rows allocated zeroed: ONE fill covers the meta words of the input level and of the pyramid built later
        bk = _Brick([e + 1 for e in extent[:3]], extent[3] + 1, n, n, dev, self._new_brick_rows(dev, clean=True), alloc=False)
        # ONE allocation and ONE fill for the directory, the bricks and the scan's scratch (round 5: two memsets)
        _, (scratch,) = _brick_arena([bk], dev)
        # the level is clamped to the EXTENT of the points, not to the layer's spatial size: a coordinate beyond
        # spatial_size (<= 65534) is a site here as it is for the hash form and the reference's InputLayer
        out_sp = tuple(max(int(k), int(e) + 1) for k, e in zip(key, extent[:3]))
        _brick_build(piece["pc"], n, 0, (1, 1, 1), (1, 1, 1), out_sp, bk, 1, scratch)
        flush_geom()
        check(lib.aabr_points_sites(piece["pc"].data_ptr(), n, bk.dims_c(), bk.dir_ptr(), bk.bricks_ptr(),
                                    ptr(piece["point_site"]), ptr(piece["first_pt"]), ptr(piece["cnt_extra"]),
                                    ptr(piece["head"]), ptr(piece["nxt"]), bk.meta.data_ptr(), 1, stream()))
        return bk, scratch

    def _finish_brick_scatter(self, pend):
        m = _collect_meta(pend)
        self._pending = None
        il = self.input
        key, n, dev, piece = il["spatial"], il["n"], pend["device"], pend["piece"]
        if m[2] == 0:
            raise _hip.AabrError("InputLayer: coordinates must lie in [0, 65534] (batch index too)")
        if il.get("bl") is not None and m[8] >= 0:
            m[11] = il.get("bl")[0] - 1                    # B samples, trailing empty ones included (flat form: the largest seen)
        if m[8] < 0:                                   # no valid point
            self.grids[key] = _Grid(torch.empty((0, 4), dtype=torch.int32, device=dev), None, 0, 0)
            il["V"] = 0
            self.input_spatial = key
            return
        if _brick_dir_words(m[8:12]) > BRICK_MAX_DIR_WORDS:
            # a few sites spread over a huge extent: the dense directory would not pay -- hash grids for this scene
            self.site_order = "first_seen"
            brick_stats["declined"] += 1
            src = il["coords_src"]
            self.input = None
            self.inputLayerEnqueue(pend["spatial_t"], pend["coords"], pend["mode"], dev, asynchronous=False,
                                   bl=pend.get("bl") is not None)
            self.input["coords_src"] = src
            return self.inputLayerFinish()
        brick_stats["built"] += 1
        bk, scratch = self._brick_scatter_launch(piece, n, key, m[8:12], dev)
        bm = _hip.read_back(bk.meta)                   # the site count sizes every later tensor
        if bm[2]:
            raise _hip.AabrError("brick grid of the input level: a point outside the directory's extent or a capacity "
                                 "overflow (meta %s)" % (bm[:4],))
        V = bm[0]
        self._brick_keep = [pend["buf"], self._brick_rows, scratch]
        self.grids[key] = _Grid(bk.coords_full[:V], None, 0, V, None, bk)
        il["V"] = V
        self.input_spatial = key

    def inputLayerFinish(self):
        """wait for the read-back (the one host sync of the input layer: V sizes every later tensor)"""
        pend = self._pending
        if pend is not None and pend.get("kind") == "brick":
            self._finish_brick_scatter(pend)
            return self.input["V"]
        if pend is not None:
            m = _collect_meta(pend)
            if pend["variant"] and m[5] == 0:
                # a point did not fit the packed word (or a hash block overflowed): the generic form on the same buffers
                scatter_stats["redone"] += 1
                pend["redo"]()
                m = _hip.read_back(pend["meta"])
            self._pending = None
            if m[2]:
                raise _hip.AabrError("InputLayer: coordinates must lie in [0, 65534] (batch index too)")
            V = m[0]
            key = self.input["spatial"]
            if self.input.get("bl") is not None and V > 0:
                m[11] = self.input.get("bl")[0] - 1        # B samples, trailing empty ones included
            if self.site_order == "brick" and V > 0 and _brick_dir_words(m[8:12]) > BRICK_MAX_DIR_WORDS:
                # a few sites spread over a huge extent: the dense directory would not pay -- hash grids for this scene
                self.site_order = "first_seen"
                brick_stats["declined"] += 1
            if self.site_order == "brick" and V > 0:
                brick_stats["built"] += 1
                self.grids[key] = self._brickify_input(pend, V, m[8:12])
            else:
                self.grids[key] = _Grid(pend["site_coords"][:V], pend["keys"], pend["cap"], V)
            self.input["V"] = V   # maxActive (meta[1]) is produced by the forward kernel: read lazily (max_active())
            self.input_spatial = key
        return self.input["V"]

    # ---- brick-major site order (extension; csrc/brick.hip) -------------------------------------------------------------
    def _brickify_input(self, pend, V, extent):
        """The voxel scatter has numbered the V input sites in first-seen order and the host knows V and the scene's extent
        (meta[8..11]).  Build the input level's brick grid from those sites, renumber them brick by brick and carry the
        input layer's per-site arrays (first point, further-point chain, point -> site) over to the new rows.  Nothing is
        read back here; the level's error flag rides with the next read (`buildBrickPyramid` / `getRuleBook`)."""
        lib = _hip.load()
        il = self.input
        dev = pend["buf"].device
        n = il["n"]
        ext = [e + 1 for e in extent[:3]]
        nsamples = extent[3] + 1
        # (rows NOT zeroed: `buildBrickPyramid` fills the ones it takes)
        bk = _Brick(ext, nsamples, V, V, dev, self._new_brick_rows(dev, clean=False))
        old_coords = pend["site_coords"]
        out_sp = tuple(max(int(k), int(e)) for k, e in zip(il["spatial"], ext))       # see _brick_scatter_launch
        scratch = _brick_build(old_coords, V, 0, (1, 1, 1), (1, 1, 1), out_sp, bk)
        flush_geom()
        nb = torch.empty(5 * V + n + 8, dtype=torch.int32, device=dev)
        new_of_old, old_of_new, first2, extra2, head2 = (nb[i * V:(i + 1) * V] for i in range(5))
        ps2 = nb[5 * V:5 * V + n]
        check(lib.aabr_brick_renumber(ptr(old_coords), V, bk.dims_c(), bk.dir_ptr(), bk.bricks_ptr(), ptr(new_of_old),
                                      ptr(old_of_new), ptr(il["first_pt"]), ptr(il["cnt_extra"]), ptr(il["head"]),
                                      ptr(first2), ptr(extra2), ptr(head2), ptr(il["point_site"]), n, ptr(ps2),
                                      bk.meta.data_ptr(), stream()))
        il.update(point_site=ps2, first_pt=first2, cnt_extra=extra2, head=head2, new_of_old=new_of_old,
                  old_of_new=old_of_new)
        self._brick_keep = [nb, self._brick_rows, scratch]
        return _Grid(bk.coords_full[:V], None, 0, V, None, bk)

    def _new_brick_rows(self, device, clean):
        """allocate the read-back block of this object's brick levels (`clean`: zeroed, so that no later level has to fill
        its row) and take row 0 for the level about to be built; returns that row's meta block"""
        self._brick_rows = (torch.zeros if clean else torch.empty)((_BK_MAX_LEVELS, _BK_ROW), dtype=torch.int32,
                                                                   device=device)
        self._brick_nrows, self._brick_rows_clean = 1, clean
        return self._brick_rows[0, 64:64 + _hip.META_WORDS]

    def _brick_read(self, post_only=False, posted=None):
        """ONE host read for every brick level enqueued since the last one: [V, per-sample offsets (64 words), meta (16)]
        per level; checks the error flags.  `post_only`: enqueue the read (a mailbox of this thread's own) and return the
        handle; `posted`: collect such a read -- the host does other work while the levels are built."""
        n = self._brick_nrows
        if posted is None:
            flush_geom()
            if post_only:
                mb = _geom_mailboxes.pop() if _geom_mailboxes else _hip.Mailbox()
                mb.post(self._brick_rows[:n].reshape(-1))
                return (mb, n)
            rows = _hip.read_back(self._brick_rows[:n].reshape(-1))
        else:
            mb, n = posted
            rows = mb.wait()
            if len(_geom_mailboxes) < 4:
                _geom_mailboxes.append(mb)
        rows = [rows[i * _BK_ROW:(i + 1) * _BK_ROW] for i in range(n)]
        for i, r in enumerate(rows):
            if r[64 + 2]:
                raise _hip.AabrError("brick grid %d: a site outside the directory's extent or a capacity overflow "
                                     "(meta %s)" % (i, r[64:64 + 4]))
        g0 = self.grids[self.input["spatial"]] if self.input is not None else None
        if g0 is not None and rows[0][64] != g0.V:    # (no input layer: the object a FullConvolution created, row 0 = its level)
            raise _hip.AabrError("brick grid of the input level holds %d sites, the voxel scatter counted %d"
                                 % (rows[0][64], g0.V))
        return rows

    def finishBrickPyramid(self):
        """collect a pyramid enqueued with `buildBrickPyramid(.., defer=True)` (no-op when there is none)"""
        pend, self._pyramid_pending = self._pyramid_pending, None
        if pend is not None:
            self._pyramid_collect(*pend)

    def buildBrickPyramid(self, specs, defer=False):
        """Extension: the strided levels of a pass as brick grids, each built from its parent LEVEL by device-side counts
        (aabr_brick_build), all enqueued back to back, ONE host read for all of their site counts and per-sample offsets.
        specs = [(out_spatial key, source spatial key, size, stride)] in dependency order."""
        self.finishBrickPyramid()
        todo = [sp for sp in specs if sp[0] not in self.grids]
        if not todo:
            return
        dev = self._brick_rows.device
        made = {}
        first_row = self._brick_nrows
        plan = []
        for osz, src, size, stride in todo:
            gs = made.get(src) or self.grids[src]
            bs = gs.brick
            ext = [min(o, (e - 1) // st_ + 1) for o, e, st_ in zip(osz, bs.ext, stride)]
            maxout = _max_outputs(size, stride)
            row = self._brick_rows[self._brick_nrows]
            self._brick_nrows += 1
            assert self._brick_nrows <= _BK_MAX_LEVELS
            bk = _Brick(ext, bs.dims[3], bs.nb_cap * maxout, bs.v_cap * maxout, dev, row[64:64 + _hip.META_WORDS], alloc=False)
            made[osz] = _Grid(None, None, 0, None, None, bk)
            plan.append((osz, bs, size, stride, bk, row))
        # ONE allocation and ONE fill for the directories, bricks and scan scratch of all the levels built here
        arena, scratch = _brick_arena([p[4] for p in plan], dev)
        if not self._brick_rows_clean:      # (rows allocated zeroed by the brick-native scatter: nothing to do)
            self._brick_rows[first_row:self._brick_nrows].zero_()
        self._brick_keep.append(arena)
        for (osz, bs, size, stride, bk, row), scr in zip(plan, scratch):
            _brick_build(bs.coords_full, bs.v_cap, bs.meta.data_ptr(), size, stride, osz, bk, 1, scr)
            _geom(G_SOFF, (MAX_SAMPLES + 1,), (bk.v_cap,), (_p(bk.coords_full), bk.meta.data_ptr(), row.data_ptr()))
        if defer:        # the levels are being built; the host collects their counts later (finishBrickPyramid)
            self._pyramid_pending = (todo, made, first_row, self._brick_read(post_only=True))
            return
        self._pyramid_collect(todo, made, first_row, None)

    def _pyramid_collect(self, todo, made, first_row, posted):
        rows = self._brick_read(posted=posted)
        for (osz, src, size, stride), r in zip(todo, rows[first_row:]):
            g = made[osz]
            V = r[0]
            off = r[1:64]
            g.V, g.coords = V, g.brick.coords_full[:V]
            g.sample_off = off if off[-1] == V else None
            self.grids[osz] = g
            self._pregrids.add(osz)

    def getSubmanifoldRuleBook(self, spatial_size, filter_size):
        """Metadata::getSubmanifoldRuleBook (Metadata.cpp:429-443) -> cached gather table"""
        k = _key(spatial_size) + _key(filter_size)
        tb = self.submanifold.get(k)
        if tb is None:
            self._materialised()
            g = self.grids[_key(spatial_size)]
            fs = _key(filter_size)
            vol = fs[0] * fs[1] * fs[2]
            dev = g.coords.device
            table = torch.empty((vol, g.V), dtype=torch.int32, device=dev)
            counts = torch.empty(vol * ((g.V + 255) // 256), dtype=torch.int32, device=dev)
            if g.V > 0 and g.brick is not None:
                _geom(G_BK_SUBM, fs, (g.V, g.brick.packed), (_p(g.coords), g.brick.level.data_ptr(), _p(table), _p(counts)))
            elif g.V > 0:
                _geom(G_SUBM, fs, (g.V, g.cap), (_p(g.coords), _p(g.keys), _p(table), _p(counts)))
            # odd filters: the input-gradient gather is the same table read with the mirrored
            # offset (u = v + off_k  <=>  v = u + off_{vol-1-k})
            tb = _Table(_Gather(table, counts, vol, g.V), None, vol, g.V, g.V,
                        flip_ok=all(f % 2 == 1 for f in fs))
            if not tb.flip_ok:
                raise NotImplementedError("even-sized submanifold filters")
            self.submanifold[k] = tb
        return tb

    def buildGridsFromInput(self, in_spatial, specs):
        """Extension: the output grids of a chain of NON-OVERLAPPING strided levels (filter size == stride at every
        level) built straight from the chain's first grid -- `specs` = [(out_spatial, composed)], composed = the
        per-axis product of the strides down to that level -- all enqueued back to back and sized by ONE read of
        their site counts (level by level every grid costs its own blocking read: 12 per FPN_Net pass).  A site of
        level k is (x >> ..) of its level-0 sites and is numbered at its first level-0 site, which is also where the
        level-by-level construction numbers it: same site lists, same order (tests compare them with the oracle's).
        `getRuleBook` picks the grids up by their spatial size."""
        gi = self.grids[_key(in_spatial)]
        if gi.brick is not None:       # brick grids: each level from the round's base with the composed stride
            return self.buildBrickPyramid([(_key(o), _key(in_spatial), _key(c), _key(c)) for o, c in specs])
        dev = gi.keys.device
        E = gi.V
        metas = torch.empty((max(len(specs), 1), _hip.META_WORDS), dtype=torch.int32, device=dev)
        ext = torch.empty((max(len(specs), 1), MAX_SAMPLES + 3), dtype=torch.int32, device=dev)
        pend = []
        for i, (osz, comp) in enumerate(specs):
            osz, comp = _key(osz), _key(comp)
            keys, cap, scratch, out_coords = _derived_level(E, dev)
            _geom(G_SITES, comp + comp + osz, (gi.V, cap),
                  (_p(gi.coords), _p(keys), _p(scratch), _p(out_coords), metas[i].data_ptr()))
            # V and the per-sample row offsets (SparseGrid::ctr) of the new grid into one row of `ext`
            _geom(G_SOFF, (MAX_SAMPLES + 1,), (max(E, 1),), (_p(out_coords), metas[i].data_ptr(), ext[i].data_ptr()))
            _keep(scratch)
            pend.append((osz, out_coords, keys, cap))
        if not pend:
            return
        _keep(metas)
        flush_geom()
        rows = ext[:len(pend)].tolist()  # the one host sync: site counts + per-sample offsets of every grid
        for (osz, out_coords, keys, cap), row in zip(pend, rows):
            V_out = row[0]
            off = row[1:]
            self.grids[osz] = _Grid(out_coords[:V_out], keys, cap, V_out,
                                    off if off[-1] == V_out else None)   # more than MAX_SAMPLES samples: no list
            self._pregrids.add(osz)

    def getRuleBook(self, in_spatial, out_spatial, filter_size, filter_stride):
        """Metadata::getRuleBook (Metadata.cpp:484-510): builds the output grid on first use."""
        k = _key(in_spatial) + _key(filter_size) + _key(filter_stride)
        tb = self.rulebooks.get(k)
        if tb is None:
            self._materialised()
            gi = self.grids[_key(in_spatial)]
            fs, st, osz = _key(filter_size), _key(filter_stride), _key(out_spatial)
            if osz in self._borrowed and osz != _key(in_spatial):
                # the input level a FullConvolution shared with this object: a convolution onto that spatial size reaches
                # other sites than the level holds, and builds its own (the reference clears and rebuilds it too,
                # ConvolutionRules.h:43-44)
                self._borrowed.discard(osz)
                del self.grids[osz]
            have = self.grids.get(osz)
            if gi.brick is not None and gi.V > 0 and osz not in self._pregrids and \
                    not (have is not None and have.brick is not None):
                self.buildBrickPyramid([(osz, _key(in_spatial), fs, st)])       # (one host read)
            elif self.site_order == "brick" and gi.V == 0:                      # an empty level under an empty level
                self.grids[osz] = _Grid(gi.coords[:0], None, 0, 0)
                tb = self.rulebooks[k] = _empty_book(fs[0] * fs[1] * fs[2], gi.coords.device)
                return tb
            go = self.grids.get(osz) if osz in self._pregrids else None
            if go is None and gi.brick is not None:
                # brick order: an output level that already exists (a second rule book onto the same output size, with
                # another filter or stride) is served from that level, as the reference serves it from its existing grid
                # (Metadata.cpp:484-510) -- rebuilding it would renumber rows that already carry features.  A brick
                # level never falls through to the hash builders below.
                go = self.grids.get(osz)
                if go is None or go.brick is None:
                    raise RuntimeError("site_order='brick': no brick level for output size %r" % (osz,))
            if go is not None:         # built ahead by buildGridsFromInput / buildBrickPyramid
                self._pregrids.discard(osz)
            else:                      # a hash level built now: the sites kernel and the host read of its site count
                flush_geom()
                keys, cap, out_coords, meta = _derived_level_now(_hip.load().aabr_convolution_sites, gi, fs, st, osz,
                                                                 gi.V * _max_outputs(fs, st))
                V_out = meta.tolist()[0]  # host sync: sizes the output feature tensor
                go = self.grids[osz] = _Grid(out_coords[:V_out], keys, cap, V_out)
            tb = self.rulebooks[k] = _strided_book(gi, go, fs, st, osz)
        return tb

    def getFullConvolutionRuleBook(self, in_spatial, out_spatial, filter_size, filter_stride, new_metadata):
        """Metadata::getFullConvolutionRuleBook (Metadata.cpp:511-531): the rule book of a FullConvolution from THIS
        object's level `in_spatial` onto a NEW level -- one site at p * stride + q for every input site p and filter offset
        q -- that is created in `new_metadata`, built once per `new_metadata`.  `new_metadata` is cleared, takes this
        object's site order and the input level (the `_Grid` object itself: it is never written) and keeps the book as its
        `fullConvolutionRuleBook`.  This object is only read.  The book is that of a Convolution from the new level down
        to the input level: `out` [vol, V_in] is complete by construction, `inn` [vol, V_new] is what the forward pass
        gathers through (as Deconvolution_updateOutput reads `tb.inn`).  First-seen order: aabr_full_convolution_sites +
        aabr_convolution_tables2 and one host read of the site count; brick order: aabr_brick_full_build +
        aabr_brick_convolution_tables, no hash builder."""
        tb = new_metadata.fullConvolutionRuleBook
        if tb is not None:
            return tb
        lib = _hip.load()
        self._materialised()
        isz, osz, fs, st = _key(in_spatial), _key(out_spatial), _key(filter_size), _key(filter_stride)
        assert len(fs) == 3 and len(st) == 3, "dimension 3 only"
        if osz != tuple((i - 1) * s_ + f for i, f, s_ in zip(isz, fs, st)):
            raise ValueError("FullConvolution: output spatial size %s is not (input %s - 1) * stride %s + filter %s"
                             % (osz, isz, st, fs))
        gi = self.grids[isz]
        dev = gi.coords.device
        vol = fs[0] * fs[1] * fs[2]
        E = gi.V * vol
        if E >= 0x7fffffff:
            raise _hip.AabrError("FullConvolution: %d input sites x filter volume %d reaches 2^31 candidate sites" % (gi.V, vol))
        flush_geom()                     # the calls below launch (and read) right away
        new_metadata.clear()
        new_metadata.site_order = self.site_order
        new_metadata.device = dev
        new_metadata.input_spatial = isz
        new_metadata.grids[isz] = gi     # (size 1 / stride 1: the new level below takes this key over, with the same rows)
        new_metadata._borrowed = {isz}   # not a level of its own making: getRuleBook does not build onto it
        big = (kMaxSpatial,) * 3         # the tables clip nothing: every site of the new level has its parent
        if gi.V == 0:
            new_metadata.grids[osz] = _Grid(gi.coords[:0], None, 0, 0) if gi.keys is None else \
                self._full_hash_level(gi, fs, st, osz, 0)
            tb = new_metadata.fullConvolutionRuleBook = _empty_book(vol, dev)
            return tb
        if gi.brick is not None:
            bs = gi.brick
            ext = [(e - 1) * s_ + f for e, f, s_ in zip(bs.ext, fs, st)]
            # bricks: bounded by the candidates, not by parent bricks * vol (a dilated 4^3 brick with size == stride == 2 touches
            # up to 27 bricks); _Brick clips both bounds to what the directory's extent can hold
            bk = _Brick(ext, bs.dims[3], E, E, dev, new_metadata._new_brick_rows(dev, clean=True), alloc=False)
            arena, (scratch,) = _brick_arena([bk], dev)                       # ONE fill: directory, bricks, scan scratch
            check(lib.aabr_brick_full_build(ptr(gi.coords), gi.V, None, _hip.i32x3(fs), _hip.i32x3(st), _hip.i32x3(osz),
                                            bk.dims_c(), bk.dir_ptr(), bk.bricks_ptr(), bk.nb_cap, bk.bcoord.data_ptr(),
                                            bk.coords_full.data_ptr(), bk.v_cap, bk.meta.data_ptr(),
                                            scratch.data_ptr(), 1, stream()))
            bm = _hip.read_back(bk.meta)         # host sync: the site count sizes the output feature tensor
            if bm[2]:
                raise _hip.AabrError("FullConvolution: a site outside the output spatial size %s, or a brick level "
                                     "overflow (meta %s)" % (osz, bm[:4]))
            V_new = bm[0]
            new_metadata._brick_keep = [new_metadata._brick_rows, arena]
            go = _Grid(bk.coords_full[:V_new], None, 0, V_new, None, bk)
        else:
            go = self._full_hash_level(gi, fs, st, osz, E)
        new_metadata.grids[osz] = go
        new_metadata._borrowed.discard(osz)
        # a Convolution's tables with the NEW level as the input side and this level as the output side
        tb = new_metadata.fullConvolutionRuleBook = _strided_book(go, gi, fs, st, big)
        return tb

    @staticmethod
    def _full_hash_level(gi, fs, st, osz, E):
        """the hash grid of the level a FullConvolution grows to, numbered first-seen (aabr_full_convolution_sites); the
        one host read of its site count (none for an empty input level)"""
        keys, cap, out_coords, meta = _derived_level_now(_hip.load().aabr_full_convolution_sites, gi, fs, st, osz, E)
        V_new = 0
        if E > 0:
            m = meta.tolist()            # host sync: sizes the output feature tensor
            if m[2]:
                raise _hip.AabrError("FullConvolution: an input site reaches outside the output spatial size %s" % (osz,))
            V_new = m[0]
        return _Grid(out_coords[:V_new], keys, cap, V_new)

    # ---- reference-format views (tests / API parity) ------------------------------------------
    def max_active(self):
        """largest number of points in one voxel (IOLayersRules.h:96-103); written by the forward kernel"""
        il = self.input
        if il.get("max_active") is None:
            if not il.get("forward_done"):
                raise _hip.AabrError("maxActive is known after InputLayer_updateOutput has run")
            il["max_active"] = max(int(il["meta"][1].item()), 0) if il["V"] else 0
        return il["max_active"]

    def inputLayerRuleBook(self):
        """[[mode, maxActive, nIn, nOut], rules V x (1+maxActive)] (IOLayersRules.h:10-15)"""
        il = self.input
        ma = self.max_active()
        w = (ma if il["mode"] in (3, 4) else 1) + 1
        rules = torch.empty((il["V"], w), dtype=torch.int32, device=il["first_pt"].device)
        check(_hip.load().aabr_input_layer_rule_table(ptr(il["first_pt"]), ptr(il["last_pt"]), ptr(il["cnt_extra"]),
                                                      ptr(il["head"]), ptr(il["nxt"]), il["V"], ma, il["mode"],
                                                      ptr(rules), stream()))
        return [il["mode"], w - 1, il["n"], il["V"]], rules

    def blLayerRuleBook(self):
        """[[mode, maxActive, B, L, V], rules int32 [V, 1 + maxActive]] (blRules, IOLayersRules.h:127-297): a row holds a
        count, then the flat point indices b * L + l it lists in ascending order (modes 1 / 2: the one point kept);
        entries past the count are unspecified.  `mode` is the BL mode the layer was built with."""
        il = self.input
        if il is None or il.get("bl") is None:
            raise _hip.AabrError("blLayerRuleBook: this Metadata was not built by a BLInputLayer (inputLayerRuleBook?)")
        head, rules = self.inputLayerRuleBook()
        return [il["bl_mode"], head[1], il["bl"][0], il["bl"][1], il["V"]], rules

    @staticmethod
    def tableToRuleBook(table):
        """gather table [vol, V] -> list over offsets of int32 [n_k, 2] (entry, row) pairs"""
        vol, V = table.shape
        rules = torch.empty((vol, max(V, 1), 2), dtype=torch.int32, device=table.device)
        counts = torch.empty(vol, dtype=torch.int32, device=table.device)
        check(_hip.load().aabr_table_to_rulebook(ptr(table), V, vol, ptr(rules), ptr(counts), stream()))
        c = counts.tolist()
        return [rules[k, : c[k]] for k in range(vol)]


def _opt(t):
    return t if (t is not None and t.numel() > 0) else None


def _featc(t, what):
    """feature matrices of the convolution / batch-norm path: fp32 (the reference's precision) or
    bf16 storage (extension, BASELINE configs 3-5; fp32 accumulation, fp32 parameters)"""
    _hip.require_gpu(t)
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("%s must be float32 or bfloat16, got %s" % (what, t.dtype))
    return t.contiguous()


def _same_dtype(a, b, what):
    if a.dtype != b.dtype:
        raise TypeError("%s: feature dtypes differ (%s vs %s)" % (what, a.dtype, b.dtype))


def _f32c(t, what):
    _hip.require_gpu(t)
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (the reference path is fp32-only, "
                        "sparseconvnet_cuda.cpp instantiates <float>), got %s" % (what, t.dtype))
    return t.contiguous()


# ------------------------------------------------------------------------------------------------
# InputLayer (pybind.cpp:154-162; sparseconvnet_cuda.cpp:432-455)
# ------------------------------------------------------------------------------------------------
def InputLayer_updateOutput(metadata, spatial_size, coords, input_features, output_features, batch_size,
                            mode):
    inp = _f32c(input_features, "input_features")
    mode = int(mode)
    if mode == 0:
        # "guaranteed unique": identical to the summing path when the guarantee holds
        V = metadata.inputLayer(spatial_size, coords, batch_size, 3, inp.device)
        if V != inp.size(0):
            raise _hip.AabrError("InputLayer mode 0 requires unique coordinates")
        metadata.input["mode"] = 3
    else:
        if mode not in (1, 2, 3, 4):
            raise ValueError("InputLayer mode must be 0..4")
        V = metadata.inputLayer(spatial_size, coords, batch_size, mode, inp.device)
    il = metadata.input
    planes = inp.size(1)
    output_features.resize_(V, planes)
    check(_hip.load().aabr_input_layer_forward(ptr(inp), ptr(output_features), V, planes, ptr(il["first_pt"]),
                                               ptr(il["cnt_extra"]), ptr(il["head"]), ptr(il["nxt"]),
                                               ptr(il["last_pt"]), il["mode"], ptr(il["meta"]), stream()))
    il["forward_done"] = True


def InputLayer_updateGradInput(metadata, d_input_features, d_output_features):
    d_out = _f32c(d_output_features, "d_output_features")
    il = metadata.input
    planes = d_out.size(1)
    d_input_features.resize_(il["n"], planes)
    check(_hip.load().aabr_input_layer_backward(ptr(d_input_features), ptr(d_out), il["n"], planes,
                                                ptr(il["point_site"]), ptr(il["first_pt"]), ptr(il["last_pt"]),
                                                ptr(il["cnt_extra"]), il["mode"], stream()))


# OutputLayer (pybind.cpp:163-170; SCN/CPU/IOLayers.cpp:95-134): the InputLayer run backwards without averaging --
# every point listed in the input rule table receives its site's row (cpu_OutputLayer_updateOutput calls
# InputLayer_BackwardPass(..., average=false)); its gradient is InputLayer_ForwardPass(..., average=false).
def OutputLayer_updateOutput(metadata, input_features, output_features):
    inp = _f32c(input_features, "input_features")
    il = metadata.input
    if il is not None and il.get("bl") is not None:
        _bl_input(metadata, "OutputLayer_updateOutput", want_bl=False)
    planes = inp.size(1)
    mode = 3 if il["mode"] == 4 else il["mode"]
    output_features.resize_(il["n"], planes)
    check(_hip.load().aabr_input_layer_backward(ptr(output_features), ptr(inp), il["n"], planes,
                                                ptr(il["point_site"]), ptr(il["first_pt"]), ptr(il["last_pt"]),
                                                ptr(il["cnt_extra"]), mode, stream()))


def OutputLayer_updateGradInput(metadata, d_input_features, d_output_features):
    d_out = _f32c(d_output_features, "d_output_features")
    il = metadata.input
    planes = d_out.size(1)
    mode = 3 if il["mode"] == 4 else il["mode"]
    d_input_features.resize_(il["V"], planes)
    check(_hip.load().aabr_input_layer_forward(ptr(d_out), ptr(d_input_features), il["V"], planes, ptr(il["first_pt"]),
                                               ptr(il["cnt_extra"]), ptr(il["head"]), ptr(il["nxt"]), None, mode,
                                               ptr(il["meta"]), stream()))


# ------------------------------------------------------------------------------------------------
# BLInputLayer / BLOutputLayer (pybind.cpp:171-187; SCN/CPU/IOLayers.cpp:138-230; blRules,
# IOLayersRules.h:127-297).  The site numbering reads the [B, L, 3] coordinates in place (csrc/point_reader.h BLReader);
# the feature passes are the flat kernels over the [B L, C] VIEW of the features -- nothing is flattened or compacted.
# ------------------------------------------------------------------------------------------------
def _bl_check(coords, input_features, mode):
    """argument refusals of BLInputLayer_updateOutput, before any launch (and before the device is asked for)"""
    if int(mode) not in BL_KERNEL_MODE:
        raise ValueError("BLInputLayer mode must be 0..4, got %r" % (mode,))
    if coords.dtype.is_floating_point or coords.dtype.is_complex or coords.dtype == torch.bool:
        raise TypeError("BLInputLayer coordinates must be an integer tensor, got %s" % coords.dtype)
    if coords.dim() != 3 or coords.size(2) != 3:
        raise ValueError("BLInputLayer coordinates must be [B, L, 3], got %s" % (tuple(coords.shape),))
    if input_features.dtype != torch.float32:
        raise TypeError("BLInputLayer features must be float32 (the reference path is fp32-only), got %s"
                        % input_features.dtype)
    if input_features.dim() != 3 or tuple(input_features.shape[:2]) != tuple(coords.shape[:2]):
        raise ValueError("BLInputLayer features must be [B, L, C] with the coordinates' B, L = %s, got %s"
                         % (tuple(coords.shape[:2]), tuple(input_features.shape)))


def _bl_input(metadata, what, want_bl=True):
    """the input-layer state of `metadata`, refusing the other form's (the reference keeps two separate rule books and
    would read an empty one)"""
    il = metadata.input
    if il is None:
        raise _hip.AabrError("%s: the Metadata holds no input layer" % what)
    if (il.get("bl") is not None) != want_bl:
        raise _hip.AabrError("%s: the Metadata was built by %s -- the two forms keep different rule books; use %s"
                             % (what, "an InputLayer" if want_bl else "a BLInputLayer",
                                "OutputLayer" if want_bl else "BLOutputLayer"))
    return il


def _bl_rows_out(il, dst, src, planes, mode):
    """dst [B, L, planes] <- the site row of every point the rule book lists, zero elsewhere: ONE launch that writes every
    element (k_voxel_backward); a layer without sites has nothing to launch over and is zeroed"""
    dst.resize_(il["bl"][0], il["bl"][1], planes)
    if il["V"] == 0:
        dst.zero_()
        return
    check(_hip.load().aabr_input_layer_backward(ptr(dst), ptr(src), il["n"], planes, ptr(il["point_site"]),
                                                ptr(il["first_pt"]), ptr(il["last_pt"]), ptr(il["cnt_extra"]), mode,
                                                stream()))


def BLInputLayer_updateOutput(metadata, spatial_size, coords, input_features, output_features, mode):
    _bl_check(coords, input_features, mode)
    inp = _f32c(input_features, "input_features")
    mode = int(mode)
    B, L, planes = inp.shape
    V = metadata.blLayer(spatial_size, coords, mode, inp.device)
    il = metadata.input
    if mode == 0 and V != B * L:
        raise _hip.AabrError("BLInputLayer mode 0 requires every row present and unique (%d sites from %d x %d rows)"
                             % (V, B, L))
    output_features.resize_(V, planes)
    check(_hip.load().aabr_input_layer_forward(ptr(inp), ptr(output_features), V, planes, ptr(il["first_pt"]),
                                               ptr(il["cnt_extra"]), ptr(il["head"]), ptr(il["nxt"]),
                                               ptr(il["last_pt"]), il["mode"], ptr(il["meta"]), stream()))
    il["forward_done"] = True


def BLInputLayer_updateGradInput(metadata, d_input_features, d_output_features):
    d_out = _f32c(d_output_features, "d_output_features")
    il = _bl_input(metadata, "BLInputLayer_updateGradInput")
    _bl_rows_out(il, d_input_features, d_out, d_out.size(1), il["mode"])


# BLOutputLayer (cpu_BLOutputLayer_updateOutput / _updateGradInput): the BL rule book run backwards without averaging -- every
# point it lists receives its site's row, every other row of [B, L, C] (empty rows included) is written as zero by the same
# kernel; its gradient is the un-averaged forward pass.
def BLOutputLayer_updateOutput(metadata, input_features, output_features):
    inp = _f32c(input_features, "input_features")
    il = _bl_input(metadata, "BLOutputLayer_updateOutput")
    _bl_rows_out(il, output_features, inp, inp.size(1), 3 if il["mode"] == 4 else il["mode"])


def BLOutputLayer_updateGradInput(metadata, d_input_features, d_output_features):
    d_out = _f32c(d_output_features, "d_output_features")
    il = _bl_input(metadata, "BLOutputLayer_updateGradInput")
    planes = d_out.size(2)
    mode = 3 if il["mode"] == 4 else il["mode"]
    d_input_features.resize_(il["V"], planes)
    check(_hip.load().aabr_input_layer_forward(ptr(d_out), ptr(d_input_features), il["V"], planes, ptr(il["first_pt"]),
                                               ptr(il["cnt_extra"]), ptr(il["head"]), ptr(il["nxt"]), None, mode,
                                               ptr(il["meta"]), stream()))


# ------------------------------------------------------------------------------------------------
# the shared gather-GEMM
# ------------------------------------------------------------------------------------------------
def _conv_fwd(inp, out, n_rows_out, gather, weight, bias, flags, pack_t=None, single=False):
    """`pack_t` (extension): a list owned by the autograd node.  The forward call (flags bit0 = 0) packs
    the weights in both orientations with one launch and leaves the input-gradient layout in it; the
    backward call (bit0 = 1) finds it there and runs without a pack launch of its own.
    `single`: the caller knows that `gather` gives every output row exactly one rule (`single_route` is asked first)."""
    lib = _hip.load()
    if weight.size(1) != 1:
        return _conv_fwd_groups(inp, out, n_rows_out, gather, weight, bias, flags)
    n_in = inp.size(1)
    w = weight.contiguous()
    if flags & 1:
        n_out = w.size(2)
        assert w.size(3) == n_in
    else:
        n_out = w.size(3)
        assert w.size(2) == n_in, (w.shape, n_in)
    assert gather.rows == n_rows_out
    _same_dtype(inp, out, "convolution")
    out.resize_(n_rows_out, n_out)
    if w.dtype != torch.float32:
        raise TypeError("convolution weights are fp32 master parameters, got %s" % w.dtype)
    bf16 = inp.dtype == torch.bfloat16
    route = single_route(n_in, n_out, inp.size(0), n_rows_out, gather.vol, bf16) if single else None
    single = route is not None
    if not single:
        route = conv_route(n_in, n_out, inp.size(0), n_rows_out, gather.vol, bf16)
    if route.kind == "narrow":
        # 32 -> 32 planes: all offsets' weights in LDS, 16 output rows per wave in registers, straight from the gather
        # table (csrc/conv_narrow.hip) -- no weight pack, no block stream
        fn = lib.aabr_conv_forward_narrow_bf16 if bf16 else lib.aabr_conv_forward_narrow
        check(fn(ptr(inp), inp.size(0), ptr(out), n_rows_out, ptr(route.stream(gather)), gather.vol, ptr(w),
                 ptr(_opt(bias)), flags & 3, stream()))
        if trace is not None:
            trace.append(("fwd", n_in, n_out, gather, inp.size(0), flags & 3, inp.dtype))
        return n_out
    if bf16:
        elems, name, dt = lib.aabr_conv_wpack_bf16_elems(gather.vol, w.size(2), w.size(3)), "wpack16", torch.bfloat16
        conv, pack2 = lib.aabr_conv_forward_bf16, lib.aabr_conv_pack_weights2_bf16
    else:
        elems, name, dt = lib.aabr_conv_wpack_floats(gather.vol, w.size(2), w.size(3)), "wpack", torch.float32
        conv, pack2 = lib.aabr_conv_forward, lib.aabr_conv_pack_weights2
    pre = getattr(weight, "_aabr_pack", None)            # WeightPackPlan: packed once per weight version
    if pre is not None and pre[0] == weight._version and pre[1] == dt and n_rows_out > 0:
        wpack = pre[3 if (flags & 1) else 2]
        if pack_t is not None and not (flags & 1):           # the node's backward pass finds its layout here
            del pack_t[:]
            pack_t.append(pre[3])
        flags |= 4
        pack_stats["plan"] += 1
    elif pack_t is not None and (flags & 1) and len(pack_t) == 1 and pack_t[0].dtype == dt:
        wpack, flags = pack_t[0], flags | 4
    else:
        wpack = _hip.workspace(name, elems, dt, inp.device)
        if pack_t is not None and not (flags & 1) and n_rows_out > 0:
            wt = torch.empty(elems, dtype=dt, device=inp.device)
            check(pack2(ptr(w), gather.vol, w.size(2), w.size(3), ptr(wpack), ptr(wt), stream()))
            del pack_t[:]
            pack_t.append(wt)
            flags |= 4
    if not (flags & 4) and n_rows_out > 0:
        pack_stats["own"] += 1                               # this call packs its weights itself
        # (the route above was asked for a packed weight: ahead of the pack, as the narrow kernel takes none)
        if not single:
            route = conv_route(n_in, n_out, inp.size(0), n_rows_out, gather.vol, bf16, prepacked=False)
    T, P = route.tile_rows, route.parts
    if route.kind in ("wide", "split", "single") and not (flags & 4):      # (fp32 storage: bf16 comes here packed only)
        # the LAUNCH's (n_in, n_out): for a transposed launch these are (w.size(3), w.size(2))
        check(lib.aabr_conv_pack_weights(ptr(w), gather.vol, n_in, n_out, flags & 1, ptr(wpack), stream()))
    blocks = ptr(route.stream(gather))
    if route.kind == "single":
        # one rule per output row: register accumulators over the offset-pair list (csrc/conv_single.hip)
        check(lib.aabr_conv_forward_single(ptr(inp), n_in, inp.size(0), ptr(out), n_out, n_rows_out, blocks, gather.vol,
                                           ptr(_opt(bias)), flags & 3, ptr(wpack), None, stream()))
    elif route.kind == "wide":
        # wide layer: big tiles, weights shared per offset (csrc/conv_wide.hip)
        fn = lib.aabr_conv_forward_wide_bf16 if bf16 else lib.aabr_conv_forward_wide
        check(fn(ptr(inp), n_in, inp.size(0), ptr(out), n_out, n_rows_out, blocks, T, gather.vol, ptr(_opt(bias)),
                 flags & 3, ptr(wpack), stream()))
    elif route.kind == "split":
        scratch = _hip.workspace("wide_split", P * n_rows_out * n_out, torch.float32, inp.device)
        if bf16:
            check(lib.aabr_conv_forward_wide_split_bf16(ptr(inp), n_in, inp.size(0), ptr(out), n_out, n_rows_out,
                                                        blocks, T, gather.vol, ptr(_opt(bias)), flags & 3, ptr(wpack),
                                                        P, ptr(scratch), stream()))
        else:
            check(lib.aabr_conv_forward_wide_split(ptr(inp), n_in, inp.size(0), ptr(out), n_out, n_rows_out, blocks,
                                                   T, gather.vol, ptr(_opt(bias)), flags & 3, ptr(wpack), None, P,
                                                   ptr(scratch), stream()))
    else:
        check(conv(ptr(inp), n_in, inp.size(0), ptr(out), n_out, n_rows_out, blocks, gather.vol,
                   ptr(w), ptr(_opt(bias)), flags, ptr(wpack), stream()))
    if trace is not None:
        trace.append(("fwd", n_in, n_out, gather, inp.size(0), flags & 3, inp.dtype))
    return n_out


def _conv_fwd_groups(inp, out, n_rows_out, gather, weight, bias, flags):
    """groups > 1 (the reference carries `groups` through every kernel: weight [vol, groups, nIn/g, nOut/g], planes
    group-major, out[:, g] = sum_k in[rule, g] @ W[k, g] -- CPU/Convolution.cpp:8-43,139-147).  Not on FPN_Net's path:
    one launch per group on contiguous copies of the group's planes, same kernels, no extra native code."""
    G = weight.size(1)
    ci, co = (weight.size(3), weight.size(2)) if flags & 1 else (weight.size(2), weight.size(3))
    assert inp.size(1) == G * ci, (inp.shape, weight.shape)
    out.resize_(n_rows_out, G * co)
    for g in range(G):
        xg = inp[:, g * ci:(g + 1) * ci].contiguous()
        og = torch.empty((n_rows_out, co), dtype=inp.dtype, device=inp.device)
        bg = bias[g * co:(g + 1) * co].contiguous() if (bias is not None and bias.numel()) else None
        _conv_fwd(xg, og, n_rows_out, gather, weight[:, g:g + 1].contiguous(), bg, flags & 3)
        out[:, g * co:(g + 1) * co] = og
    return G * co


pack_stats = {"plan": 0, "own": 0}   # convolution launches served by a WeightPackPlan / packing on their own


class WeightPackPlan:
    """Extension (the reference's GEMMs read W[k] in place): the packed copies of EVERY convolution weight of a
    network -- forward layout and input-gradient layout -- produced by ONE launch per forward pass
    (`aabr_conv_pack_weights_jobs`) instead of one pack launch per layer call.  `refresh()` packs and leaves each
    weight's packs on the parameter (`_aabr_pack`) for `_conv_fwd` to pick up; `release()` takes them away again
    when the forward pass is over (the autograd nodes keep the input-gradient packs they need), so a layer called
    on its own later -- possibly after an optimizer changed the weights through `.data`, which no version counter
    sees -- never meets a stale pack."""

    def __init__(self, weights, dtype):
        assert dtype in (torch.float32, torch.bfloat16)
        self.weights = [w for w in weights if w.is_cuda]
        self.dtype = dtype
        self._ptrs = None

    def _build(self):
        import struct
        lib = _hip.load()
        dev = self.weights[0].device
        es = 4 if self.dtype == torch.float32 else 2
        offs, total, blocks = [], 0, [0]
        for w in self.weights:
            assert w.dim() == 4 and w.size(1) == 1 and w.dtype == torch.float32 and w.is_contiguous()
            e = int(lib.aabr_conv_wpack_floats(w.size(0), w.size(2), w.size(3)))
            e = (e + 63) // 64 * 64                              # every pack 16-byte aligned in the arena
            offs.append((total, total + e, e))
            total += 2 * e
            blocks.append(blocks[-1] + int(lib.aabr_conv_pack_job_blocks(w.size(0), w.size(2), w.size(3))))
        self.arena = torch.empty(total, dtype=self.dtype, device=dev)
        base = self.arena.data_ptr()
        rec = b""
        self.packs = []
        for w, (f, t, e), b in zip(self.weights, offs, blocks):
            rec += struct.pack("<QQQiiiiq", w.data_ptr(), base + f * es, base + t * es, w.size(0), w.size(2), w.size(3),
                               0 if self.dtype == torch.float32 else 1, b)
            self.packs.append((self.arena[f:f + e], self.arena[t:t + e]))
        self.jobs = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to(dev)
        self.total_blocks = blocks[-1]
        self._ptrs = [w.data_ptr() for w in self.weights]

    def refresh(self):
        if not self.weights:
            return
        if [w.data_ptr() for w in self.weights] != self._ptrs:
            self._build()
        check(_hip.load().aabr_conv_pack_weights_jobs(ptr(self.jobs), len(self.weights), self.total_blocks, stream()))
        for w, (pf, pt) in zip(self.weights, self.packs):
            w._aabr_pack = (w._version, self.dtype, pf, pt)

    def release(self):
        for w in self.weights:
            if hasattr(w, "_aabr_pack"):
                del w._aabr_pack


def wide_tile_rows(n_in, n_out, rows_in, rows_out, vol, bf16=False, prepacked=True):
    """rows per tile when this launch can go to the wide-layer kernel (csrc/conv_wide.hip), else 0.  bf16 storage: only
    with a prepacked weight (the training path always has one; a stand-alone call packs inside the 64-row-tile entry)."""
    if rows_out == 0:
        return 0
    lib = _hip.load()
    if bf16:
        return lib.aabr_conv_wide_tile_rows_bf16(n_in, n_out, rows_in, rows_out, vol) if prepacked else 0
    return lib.aabr_conv_wide_tile_rows(n_in, n_out, rows_in, rows_out, vol)


def narrow_ok(n_in, n_out, rows_in, rows_out, vol, bf16):
    """True when this launch can go to the 32 -> 32 kernel (csrc/conv_narrow.hip); asked first by `conv_route`"""
    if rows_out == 0:
        return False
    return bool(_hip.load().aabr_conv_narrow_ok(n_in, n_out, rows_in, rows_out, vol, 1 if bf16 else 0))


def wide_split(n_in, n_out, rows_in, rows_out, vol, bf16=False):
    """(tile_rows, parts) when this launch can go to the offset-split form of the wide kernel (coarse maps: too few
    (tile, slab) items to fill the chip; csrc/conv_wide.hip aabr_conv_forward_wide_split), else None"""
    if rows_out == 0:
        return None
    lib = _hip.load()
    v = (lib.aabr_conv_wide_split_bf16 if bf16 else lib.aabr_conv_wide_split)(n_in, n_out, rows_in, rows_out, vol)
    return (v & 0xffff, v >> 16) if v else None


class ConvRoute(collections.namedtuple("ConvRoute", "kind tile_rows parts bf16")):
    """What `conv_route` decided for one forward-form launch: `kind` None (no output rows), "narrow", "wide", "split"
    or "tiles"; `tile_rows` T of "wide" / "split" and `parts` P of "split", else 0; `bf16` the feature storage.
    `single_route` returns kind "single" (k_conv_single over the offset pairs) or None; `single_bwd_stats_route` the same
    kind with `parts` = the backward-statistics parts its write-out forms."""
    __slots__ = ()

    def stream(self, gather):
        """the structure of `gather` the launch reads, built on first use (a launch without rows: the tile blocks)"""
        if self.kind == "narrow":
            return gather.table
        if self.kind == "single":
            return gather.pairs()
        if self.kind in ("wide", "split"):
            return gather.blocks_wide(self.tile_rows)
        return gather.blocks()

    @property
    def takes_residual(self):
        """the launch can add a residual in its write-out (the split's second stage, k_split_reduce, adds it)"""
        return self.kind in ("wide", "split", "single")

    def stats_parts(self, rows_out):
        """BatchNorm partial sums the launch's write-out can form over its `rows_out` rows -- one per tile of >= 64
        rows (a smaller WIDE_ROWS tile does not), one per workgroup of the bf16 narrow kernel -- or 0"""
        if self.kind == "wide" and self.tile_rows >= 64:
            return (rows_out + self.tile_rows - 1) // self.tile_rows
        if self.kind == "narrow" and self.bf16:
            return int(_hip.load().aabr_conv_narrow_parts(rows_out))
        if self.kind == "single":         # `single_bwd_stats_route`: one part per chunk of the pair list; else 0
            return self.parts
        return 0


def conv_route(n_in, n_out, rows_in, rows_out, vol, bf16, prepacked=True, residual=False):
    """The kernel family of a forward-form launch, read by `_conv_fwd`, `compile_streams` and planExecutor alike.  In
    order: "narrow" (the 32 -> 32 kernel, csrc/conv_narrow.hip; not when a `residual` is to ride in the write-out),
    "wide" (k_conv_cs, csrc/conv_wide.hip), "split" (its offset-split form), "tiles" (the 64-row-tile kernels of
    aabr_conv_forward[_bf16]); bf16 storage takes "wide" or "split" only with a `prepacked` weight."""
    if rows_out == 0:
        return ConvRoute(None, 0, 0, bf16)
    if not residual and narrow_ok(n_in, n_out, rows_in, rows_out, vol, bf16):
        return ConvRoute("narrow", 0, 0, bf16)
    T = wide_tile_rows(n_in, n_out, rows_in, rows_out, vol, bf16, prepacked)
    if T:
        return ConvRoute("wide", T, 0, bf16)
    sp = wide_split(n_in, n_out, rows_in, rows_out, vol, bf16) if (prepacked or not bf16) else None
    return ConvRoute("split", sp[0], sp[1], bf16) if sp else ConvRoute("tiles", 0, 0, bf16)


def single_route(n_in, n_out, rows_in, rows_out, vol, bf16, stats=False):
    """Asked BEFORE `conv_route`, and only by callers that know by construction that every output row of the launch's rule
    book has exactly one rule (a SubmanifoldConvolution of filter volume 1, forward and input gradient; a Deconvolution with
    filter == stride, forward): ConvRoute("single") when the launch should go to k_conv_single (csrc/conv_single.hip,
    decided by csrc/conv_single_tiles.h: fp32 storage, no BatchNorm statistics wanted from the write-out -- `stats` --,
    n_in <= 128, enough rows, knob CONV_SINGLE), else None.  The route takes a packed weight and a residual."""
    if rows_out == 0:
        return None
    if not _hip.load().aabr_conv_single_chunk(n_in, n_out, rows_in, rows_out, vol, 1 if bf16 else 0, 1 if stats else 0):
        return None
    return ConvRoute("single", 0, 0, bf16)


def single_bwd_stats_route(n_in, n_out, rows_in, rows_out, vol, bf16):
    """Asked before `single_route(..., stats=True)` (which keeps refusing) for an INPUT-GRADIENT launch with one rule per
    output row whose write-out owes the BatchNorm behind it its backward statistics -- the input gradient of a Convolution
    with filter == stride: ConvRoute("single") with `parts` = the fp64 parts k_conv_single<KG, true> writes (one per chunk
    of the pair list, `stats_parts`), when csrc/conv_single_tiles.h's `single_bwd_stats_refusal` lets it through (the
    conditions of `single_route` but the statistics one, knob SINGLE_BWD_STATS), else None."""
    if rows_out == 0:
        return None
    lib = _hip.load()
    chunk = lib.aabr_conv_single_bwd_stats_chunk(n_in, n_out, rows_in, rows_out, vol, 1 if bf16 else 0)
    if not chunk:
        return None
    return ConvRoute("single", 0, int(lib.aabr_conv_single_bwd_stats_parts(rows_out, vol, chunk)), bf16)


def _conv_dw(inp, d_out, gather, d_weight, d_bias):
    lib = _hip.load()
    if d_weight.dim() == 4 and d_weight.size(1) != 1:     # groups: one launch per group (see _conv_fwd_groups)
        G, ci, co = d_weight.size(1), d_weight.size(2), d_weight.size(3)
        for g in range(G):
            dwg = torch.zeros((d_weight.size(0), 1, ci, co), dtype=d_weight.dtype, device=d_weight.device)
            dbg = torch.zeros(co, dtype=d_bias.dtype, device=d_bias.device) if (d_bias is not None and d_bias.numel()) \
                else None
            _conv_dw(inp[:, g * ci:(g + 1) * ci].contiguous(), d_out[:, g * co:(g + 1) * co].contiguous(), gather, dwg, dbg)
            d_weight[:, g] = dwg[:, 0]
            if dbg is not None:
                d_bias[g * co:(g + 1) * co] = dbg
        return
    n_in, n_out, V_out = inp.size(1), d_out.size(1), d_out.size(0)
    assert gather.rows == V_out
    assert d_weight.is_contiguous() and d_weight.numel() == gather.vol * n_in * n_out
    pairs = gather.pairs()
    mc = gather.max_chunks(n_in, n_out)
    scratch = _hip.workspace("dw", lib.aabr_conv_dw_scratch_floats(mc, n_in, n_out), torch.float32, inp.device)
    _same_dtype(inp, d_out, "convolution backward")
    fn = lib.aabr_conv_backward_weight_bf16 if inp.dtype == torch.bfloat16 else lib.aabr_conv_backward_weight
    check(fn(ptr(inp), n_in, ptr(d_out), n_out, V_out, ptr(pairs), gather.vol, mc,
             ptr(d_weight), ptr(_opt(d_bias)), ptr(scratch), stream()))
    if trace is not None:
        trace.append(("dw", n_in, n_out, gather, inp.size(0), 0, inp.dtype))


def compile_streams(gather, rows_in, n_in, n_out, dtype, weight_grad=False, single=False, single_bwd_stats=False):
    """Build, ahead of their first use, the block stream the forward-form launch (n_in -> n_out over `gather`) will
    read (its `conv_route`, for a prepacked weight) -- and, with `weight_grad`, the offset-pair lists of the dW kernel.
    `single`: the book gives every output row one rule (see `single_route`, asked first: such a launch reads the pairs).
    `single_bwd_stats`: an input-gradient launch over such a book that may owe a BatchNorm its backward statistics
    (`single_bwd_stats_route`): the pairs as well as the stream of its `conv_route`, which it takes when nothing claims them."""
    if gather is None or gather.rows == 0:
        return
    bf16 = dtype == torch.bfloat16
    route = single_route(n_in, n_out, rows_in, gather.rows, gather.vol, bf16) if single else None
    (route or conv_route(n_in, n_out, rows_in, gather.rows, gather.vol, bf16)).stream(gather)
    if weight_grad or (single_bwd_stats and
                       single_bwd_stats_route(n_in, n_out, rows_in, gather.rows, gather.vol, bf16) is not None):
        gather.pairs()


def _macs(tb, weight):
    if not count_macs:
        return 0.0
    return LazyMacs([tb.out.total_slot() + (float(weight.size(2) * weight.size(3) * weight.size(1)),)])


# SubmanifoldConvolution (pybind.cpp:134-143)
def SubmanifoldConvolution_updateOutput(spatial_size, filter_size, metadata, input_features, output_features,
                                        weight, bias, pack_t=None):
    inp = _featc(input_features, "input_features")
    tb = metadata.getSubmanifoldRuleBook(spatial_size, filter_size)
    _conv_fwd(inp, output_features, tb.V_out, tb.out, weight, bias, 0, pack_t, single=tb.vol == 1)
    return _macs(tb, weight)


def SubmanifoldConvolution_backward(spatial_size, filter_size, metadata, input_features, d_input_features,
                                    d_output_features, weight, d_weight, d_bias, pack_t=None, need_d_input=True):
    inp = _featc(input_features, "input_features")
    d_out = _featc(d_output_features, "d_output_features")
    tb = metadata.getSubmanifoldRuleBook(spatial_size, filter_size)
    if need_d_input:  # d_in[u] = sum_k d_out[table[k'][u]] @ W[vol-1-k']^T  (flags: transpose | mirrored offset)
        _conv_fwd(d_out, d_input_features, tb.V_in, tb.out, weight, None, 1 | 2, pack_t, single=tb.vol == 1)
    _conv_dw(inp, d_out, tb.out, d_weight, d_bias)


# Convolution (pybind.cpp:54-65)
def Convolution_updateOutput(input_size, output_size, filter_size, filter_stride, metadata, input_features,
                             output_features, weight, bias, pack_t=None):
    inp = _featc(input_features, "input_features")
    tb = metadata.getRuleBook(input_size, output_size, filter_size, filter_stride)
    _conv_fwd(inp, output_features, tb.V_out, tb.out, weight, bias, 0, pack_t)
    return _macs(tb, weight)


def Convolution_backward(input_size, output_size, filter_size, filter_stride, metadata, input_features,
                         d_input_features, d_output_features, weight, d_weight, d_bias, pack_t=None, need_d_input=True):
    inp = _featc(input_features, "input_features")
    d_out = _featc(d_output_features, "d_output_features")
    tb = metadata.getRuleBook(input_size, output_size, filter_size, filter_stride)
    if need_d_input:
        _conv_fwd(d_out, d_input_features, tb.V_in, tb.inn, weight, None, 1, pack_t)
    _conv_dw(inp, d_out, tb.out, d_weight, d_bias)


# Deconvolution (pybind.cpp:78-89): the rule book is looked up as (outputSize, inputSize) with
# the columns swapped (CPU/Deconvolution.cpp:15-16,34-37)
def Deconvolution_updateOutput(input_size, output_size, filter_size, filter_stride, metadata, input_features,
                               output_features, weight, bias, pack_t=None):
    inp = _featc(input_features, "input_features")
    tb = metadata.getRuleBook(output_size, input_size, filter_size, filter_stride)
    # filter == stride: every output site has one parent site at one offset
    _conv_fwd(inp, output_features, tb.V_in, tb.inn, weight, bias, 0, pack_t,
              single=_key(filter_size) == _key(filter_stride))
    return _macs(tb, weight)


def Deconvolution_backward(input_size, output_size, filter_size, filter_stride, metadata, input_features,
                           d_input_features, d_output_features, weight, d_weight, d_bias, pack_t=None, need_d_input=True):
    inp = _featc(input_features, "input_features")
    d_out = _featc(d_output_features, "d_output_features")
    tb = metadata.getRuleBook(output_size, input_size, filter_size, filter_stride)
    if need_d_input:
        _conv_fwd(d_out, d_input_features, tb.V_out, tb.out, weight, None, 1, pack_t)
    _conv_dw(inp, d_out, tb.inn, d_weight, d_bias)


# FullConvolution / TransposeConvolution (pybind.cpp:90-101; CPU/Convolution.cpp:255-329): the arithmetic of a
# Deconvolution -- out[p * stride + q] += in[p] @ W[q] -- onto a level that `mIn.getFullConvolutionRuleBook` creates in
# `mOut`; every convolution kernel runs unchanged on that book's tables.
def FullConvolution_updateOutput(input_size, output_size, filter_size, filter_stride, mIn, mOut, input_features,
                                 output_features, weight, bias, pack_t=None):
    inp = _featc(input_features, "input_features")
    tb = mIn.getFullConvolutionRuleBook(input_size, output_size, filter_size, filter_stride, mOut)
    if tb.V_in == 0:                                    # no input site, no output site
        output_features.resize_(0, weight.size(1) * weight.size(3))
        return 0.0
    # filter == stride: the regions are disjoint, every new site has one parent site at one offset
    _conv_fwd(inp, output_features, tb.V_in, tb.inn, weight, bias, 0, pack_t,
              single=_key(filter_size) == _key(filter_stride))
    return _macs(tb, weight)


def FullConvolution_backward(input_size, output_size, filter_size, filter_stride, mIn, mOut, input_features,
                             d_input_features, d_output_features, weight, d_weight, d_bias, pack_t=None,
                             need_d_input=True):
    inp = _featc(input_features, "input_features")
    d_out = _featc(d_output_features, "d_output_features")
    tb = mIn.getFullConvolutionRuleBook(input_size, output_size, filter_size, filter_stride, mOut)
    if tb.V_in == 0:
        d_input_features.resize_(0, weight.size(1) * weight.size(2))
        d_weight.zero_()
        if d_bias is not None and d_bias.numel():
            d_bias.zero_()
        return
    if need_d_input:
        _conv_fwd(d_out, d_input_features, tb.V_out, tb.out, weight, None, 1, pack_t)
    _conv_dw(inp, d_out, tb.inn, d_weight, d_bias)


# ------------------------------------------------------------------------------------------------
# BatchNormalization (pybind.cpp:219-221; batchNormalization.py:120-171)
# ------------------------------------------------------------------------------------------------
def BatchNormalization_updateOutput(input_features, output_features, saveMean, saveInvStd, runningMean,
                                    runningVar, weight, bias, eps, momentum, train, leakiness):
    inp = _featc(input_features, "input_features")
    lib = _hip.load()
    output_features.resize_as_(inp)
    if inp.dim() != 2:
        return
    rows, planes = inp.shape
    for t_, nm_ in ((saveMean, "saveMean"), (saveInvStd, "saveInvStd"), (runningMean, "runningMean"),
                    (runningVar, "runningVar")):
        if t_.dtype != torch.float32 or t_.numel() < planes:
            raise TypeError("BatchNormalization: %s must hold %d float32 values, got %s[%d]"
                            % (nm_, planes, t_.dtype, t_.numel()))
    scratch = _hip.workspace("bn", lib.aabr_bn_scratch_floats(planes), torch.float32, inp.device)
    _same_dtype(inp, output_features, "BatchNormalization")
    fn = lib.aabr_bn_forward_bf16 if inp.dtype == torch.bfloat16 else lib.aabr_bn_forward
    check(fn(ptr(inp), ptr(output_features), rows, planes, ptr(saveMean), ptr(saveInvStd),
                              ptr(runningMean), ptr(runningVar), ptr(_opt(weight)), ptr(_opt(bias)), float(eps),
                              float(momentum), int(bool(train)), float(leakiness), ptr(scratch), stream()))


def BatchNormalization_backward(input_features, d_input_features, output_features, d_output_features, saveMean,
                                saveInvStd, runningMean, runningVar, weight, bias, d_weight, d_bias, leakiness):
    """NB: the reference overwrites d_output_features in place with the activation-masked
    gradient (CPU/BatchNormalization.cpp:79-82); nothing downstream reads it, so this
    implementation leaves it untouched (one HBM write pass saved)."""
    inp = _featc(input_features, "input_features")
    d_out = _featc(d_output_features, "d_output_features")
    lib = _hip.load()
    d_input_features.resize_as_(inp)
    if inp.dim() != 2:
        return
    rows, planes = inp.shape
    scratch = _hip.workspace("bn", lib.aabr_bn_scratch_floats(planes), torch.float32, inp.device)
    _same_dtype(inp, d_out, "BatchNormalization backward")
    _same_dtype(inp, output_features, "BatchNormalization backward")
    fn = lib.aabr_bn_backward_bf16 if inp.dtype == torch.bfloat16 else lib.aabr_bn_backward
    check(fn(ptr(inp), ptr(d_input_features), ptr(output_features.contiguous()), ptr(d_out),
                               rows, planes, ptr(saveMean), ptr(saveInvStd), ptr(_opt(weight)), ptr(_opt(bias)),
                               ptr(_opt(d_weight)), ptr(_opt(d_bias)), float(leakiness), ptr(scratch), stream()))


# ------------------------------------------------------------------------------------------------
# SparseToDense (pybind.cpp:124-133; SCN/CPU/SparseToDense.cpp:36-87)
# ------------------------------------------------------------------------------------------------
def _batch_size(metadata):
    """number of samples = size of the per-sample grid vector in the reference
    (`m.grids.begin()->second.size()`, SparseToDense.cpp:43); one small read-back, cached"""
    bs = metadata._batch_size_cache
    if bs is None:
        g = metadata.grids[metadata.input_spatial]
        bs = int(g.coords[:, 3].max().item()) + 1 if g.V else 0
        metadata._batch_size_cache = bs
    return bs


def SparseToDense_updateOutput(spatial_size, metadata, input_features, output_features, nPlanes):
    inp = _f32c(input_features, "input_features")
    g = metadata.grids[_key(spatial_size)]
    sp = _key(spatial_size)
    bs = _batch_size(metadata)
    output_features.resize_(bs, int(nPlanes), *sp)
    check(_hip.load().aabr_sparse_to_dense_forward(ptr(g.coords), g.V, ptr(inp), inp.size(1) if inp.dim() == 2 else
                                                   int(nPlanes), _hip.i32x3(sp), bs, ptr(output_features),
                                                   stream()))


def SparseToDense_updateGradInput(spatial_size, metadata, input_features, d_input_features, d_output_features):
    d_out = _f32c(d_output_features, "d_output_features")
    g = metadata.grids[_key(spatial_size)]
    d_input_features.resize_as_(input_features)
    if input_features.dim() != 2:
        return
    check(_hip.load().aabr_sparse_to_dense_backward(ptr(g.coords), g.V, ptr(d_input_features),
                                                    input_features.size(1), _hip.i32x3(_key(spatial_size)),
                                                    ptr(d_out), stream()))


# ------------------------------------------------------------------------------------------------
# MaxPooling / AveragePooling / UnPooling (pybind.cpp:33-53,171-180; SCN/CPU/MaxPooling.cpp, AveragePooling.cpp,
# UnPooling.cpp): csrc/pool.hip -- every pass is ONE gather launch over one table of the strided rule book, which is cached
# under the key of a Convolution of that size and stride (a pooling layer and a strided convolution onto the same level
# share grid and tables).
# ------------------------------------------------------------------------------------------------
POOL_MAX0, POOL_SUM = 0, 1     # csrc/pool.hip modes


def _pool_drop(features, nFeaturesToDrop, what):
    drop = int(nFeaturesToDrop)
    if features.dim() != 2 or not 0 <= drop < features.size(1):
        raise ValueError("%s: nFeaturesToDrop = %d of a feature matrix of shape %s" % (what, drop, tuple(features.shape)))
    return drop


def _pool_gather(src, col0, planes, gather, mode, div, dst, dst_col0, dst_width):
    """dst[gather.rows, dst_width] <- the reduction of src[:, col0:col0 + planes] over `gather` (one launch; none for an
    empty destination)"""
    _same_dtype(src, dst, "pooling")
    dst.resize_(gather.rows, dst_width)
    if gather.rows == 0:
        return
    flush_geom()
    check(_hip.load().aabr_pool_gather(ptr(src), int(src.dtype == torch.bfloat16), src.size(1), col0, planes,
                                       ptr(gather.table), gather.vol, gather.rows, mode, float(div), ptr(dst), dst_width,
                                       dst_col0, dst_width, stream()))


def MaxPooling_updateOutput(inputSize, outputSize, poolSize, poolStride, metadata, input_features, output_features,
                            nFeaturesToDrop):
    inp = _featc(input_features, "input_features")
    drop = _pool_drop(inp, nFeaturesToDrop, "MaxPooling")
    tb = metadata.getRuleBook(inputSize, outputSize, poolSize, poolStride)
    _pool_gather(inp, drop, inp.size(1) - drop, tb.out, POOL_MAX0, 0.0, output_features, 0, inp.size(1) - drop)


def MaxPooling_updateGradInput(inputSize, outputSize, poolSize, poolStride, metadata, input_features, d_input_features,
                               output_features, d_output_features, nFeaturesToDrop):
    """every input that equals its window's output receives the window's gradient; the comparison is on the columns the
    forward pass read (the reference's CPU kernel compares unshifted columns when nFeaturesToDrop > 0: not reproduced)"""
    inp = _featc(input_features, "input_features")
    out = _featc(output_features, "output_features")
    d_out = _featc(d_output_features, "d_output_features")
    drop = _pool_drop(inp, nFeaturesToDrop, "MaxPooling")
    planes = inp.size(1) - drop
    _same_dtype(inp, out, "MaxPooling backward")
    _same_dtype(inp, d_out, "MaxPooling backward")
    _same_dtype(inp, d_input_features, "MaxPooling backward")
    tb = metadata.getRuleBook(inputSize, outputSize, poolSize, poolStride)
    if tuple(out.shape) != (tb.V_out, planes) or tuple(d_out.shape) != (tb.V_out, planes) or inp.size(0) != tb.V_in:
        raise ValueError("MaxPooling backward: shapes %s / %s / %s do not fit the rule book (%d -> %d rows, %d planes)"
                         % (tuple(inp.shape), tuple(out.shape), tuple(d_out.shape), tb.V_in, tb.V_out, planes))
    d_input_features.resize_(tb.V_in, inp.size(1))
    if tb.V_in == 0:
        return
    flush_geom()
    check(_hip.load().aabr_pool_max_backward(ptr(inp), ptr(out), ptr(d_out), int(inp.dtype == torch.bfloat16), inp.size(1),
                                             drop, planes, ptr(tb.inn.table), tb.vol, tb.V_in, ptr(d_input_features),
                                             stream()))


def AveragePooling_updateOutput(inputSize, outputSize, poolSize, poolStride, metadata, input_features, output_features,
                                nFeaturesToDrop):
    inp = _featc(input_features, "input_features")
    drop = _pool_drop(inp, nFeaturesToDrop, "AveragePooling")
    tb = metadata.getRuleBook(inputSize, outputSize, poolSize, poolStride)
    _pool_gather(inp, drop, inp.size(1) - drop, tb.out, POOL_SUM, tb.vol, output_features, 0, inp.size(1) - drop)


def AveragePooling_updateGradInput(inputSize, outputSize, poolSize, poolStride, metadata, input_features,
                                   d_input_features, d_output_features, nFeaturesToDrop):
    d_out = _featc(d_output_features, "d_output_features")
    drop = _pool_drop(input_features, nFeaturesToDrop, "AveragePooling")
    planes = input_features.size(1) - drop
    tb = metadata.getRuleBook(inputSize, outputSize, poolSize, poolStride)
    if tuple(d_out.shape) != (tb.V_out, planes) or input_features.size(0) != tb.V_in:
        raise ValueError("AveragePooling backward: shapes %s / %s do not fit the rule book (%d -> %d rows, %d planes)"
                         % (tuple(input_features.shape), tuple(d_out.shape), tb.V_in, tb.V_out, planes))
    _pool_gather(d_out, 0, planes, tb.inn, POOL_SUM, tb.vol, d_input_features, drop, input_features.size(1))


def _unpool_book(outputSize, inputSize, poolSize, poolStride, metadata):
    """the book (fine, coarse, size, stride) an UnPooling from the coarse level `inputSize` reads; the fine level must exist"""
    metadata._materialised()
    if _key(outputSize) not in metadata.grids:
        raise RuntimeError("UnPooling: the metadata holds no level of spatial size %s to unpool onto (UnPooling returns to "
                           "a level that a pooling or a strided convolution has come from)" % (list(_key(outputSize)),))
    return metadata.getRuleBook(outputSize, inputSize, poolSize, poolStride)


def UnPooling_updateOutput(inputSize, outputSize, poolSize, poolStride, metadata, input_features, output_features,
                           nFeaturesToDrop):
    inp = _featc(input_features, "input_features")
    drop = _pool_drop(inp, nFeaturesToDrop, "UnPooling")
    tb = _unpool_book(outputSize, inputSize, poolSize, poolStride, metadata)
    if inp.size(0) != tb.V_out:
        raise ValueError("UnPooling: %d feature rows on a level of %d sites" % (inp.size(0), tb.V_out))
    _pool_gather(inp, drop, inp.size(1) - drop, tb.inn, POOL_SUM, 0.0, output_features, 0, inp.size(1) - drop)


def UnPooling_updateGradInput(inputSize, outputSize, poolSize, poolStride, metadata, d_input_features, d_output_features,
                              nFeaturesToDrop):
    """`d_input_features` arrives with the input's shape (unPooling.py sizes it); every element of it is written"""
    d_out = _featc(d_output_features, "d_output_features")
    drop = _pool_drop(d_input_features, nFeaturesToDrop, "UnPooling")
    planes = d_input_features.size(1) - drop
    tb = _unpool_book(outputSize, inputSize, poolSize, poolStride, metadata)
    if tuple(d_out.shape) != (tb.V_in, planes) or d_input_features.size(0) != tb.V_out:
        raise ValueError("UnPooling backward: shapes %s / %s do not fit the rule book (%d <- %d rows, %d planes)"
                         % (tuple(d_input_features.shape), tuple(d_out.shape), tb.V_out, tb.V_in, planes))
    _pool_gather(d_out, 0, planes, tb.out, POOL_SUM, 0.0, d_input_features, drop, d_input_features.size(1))
