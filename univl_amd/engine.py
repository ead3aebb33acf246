"""Flat parameter storage and static execution plans for the UniVL hot path.

Design (MI355X-first):
  * all parameters live in ONE flat fp32 buffer (plus a flat fp32 gradient buffer and, in bf16 mode, a flat bf16
    shadow the GEMMs read); `nn.Parameter`s are views into it, so the reference's names/shapes/state_dict are
    preserved while query/key/value become one [2304,768] operand, the optimizer is one streaming kernel, and a
    data-parallel bucket is one contiguous slice.
  * shapes on this path are static (fixed max_words/max_frames, drop_last batches), so a forward/backward is a
    STATIC PLAN: a list of pre-built C descriptors pointing into a persistent workspace.  Running a plan only
    enqueues kernels on the current HIP stream; it is what gets captured into a hipGraph.
"""
import contextlib
import ctypes as C
import gc
import os
import weakref

import torch

from . import _ab, _lib, ops

@contextlib.contextmanager
def no_gc():
    """hipGraph capture must not be interrupted by Python's cyclic garbage collector: a collection that happens to run inside
    a capture frees device tensors / events of unrelated dead objects (an earlier model, old plans), which is illegal while
    a stream is capturing and aborts the process."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


GUARDED = []          # UNIVL_GUARD=1 (debugging): (tag, base tensor, guard elements, payload elements) of every workspace


def _workspace(dev, zeros=False):
    """Allocator of the persistent workspaces.  Debugging switches: UNIVL_POISON=1 fills floating-point buffers with NaN, so
    that a kernel reading something no kernel has written yet shows up in the outputs instead of depending on what the
    caching allocator happens to hand back; UNIVL_GUARD=1 puts a sentinel band before and after every buffer
    (check_guards() reports the buffers whose neighbourhood a kernel wrote into)."""
    poison = bool(_ab.get("poison")) and not zeros
    guard = bool(_ab.get("guard"))

    def e(*s, dtype=torch.float32):
        shape = tuple(s[0]) if (len(s) == 1 and isinstance(s[0], (tuple, list))) else tuple(s)
        n = 1
        for d in shape:
            n *= d
        if guard:
            G = 1024
            base = torch.empty(n + 2 * G, device=dev, dtype=dtype)
            base.view(torch.uint8).fill_(0xA5)
            t = base[G:G + n].view(shape)
            import traceback
            GUARDED.append(("%s %s @%s" % (shape, dtype, traceback.extract_stack(limit=3)[0].lineno), base, G, n))
        else:
            t = torch.empty(shape, device=dev, dtype=dtype)
        if zeros:
            t.zero_()
        elif poison and dtype.is_floating_point:
            t.fill_(float("nan"))
        return t
    return e


def check_guards():
    bad = []
    for tag, base, G, n in GUARDED:
        raw = base.view(torch.uint8)
        esz = base.element_size()
        lo, hi = raw[:G * esz], raw[(G + n) * esz:]
        if bool((lo != 0xA5).any()) or bool((hi != 0xA5).any()):
            bad.append((tag, int((lo != 0xA5).sum()), int((hi != 0xA5).sum())))
    return bad


_ALIGN = 64  # elements; keeps every tensor 256-byte aligned in fp32 and 128-byte in bf16
FLAT_REGISTRY = weakref.WeakSet()   # lets the fused optimizer find the flat buffers that own a Parameter


def _is_atomic_region(name, shape):
    """Region V: tensors whose gradients are produced by atomics / scatter-add (embedding tables, all vectors)."""
    if len(shape) == 1:
        return True
    if "embeddings" in name and not name.startswith("visual.embeddings.word_embeddings"):
        return True
    if name.startswith("similarity_dense"):
        return True
    return False


class FlatParams:
    """Owns p32 / g32 (/ p16) and re-points the module's Parameters at views of p32."""

    def __init__(self, named_params, device, compute_dtype):
        self.device = torch.device(device)
        self.compute_dtype = compute_dtype
        self.dt = ops.dtype_code(compute_dtype)
        names_v = [(n, p) for n, p in named_params if _is_atomic_region(n, tuple(p.shape))]
        names_m = [(n, p) for n, p in named_params if not _is_atomic_region(n, tuple(p.shape))]
        self.index = {}
        off = 0
        for n, p in names_v + names_m:
            if n == (names_m[0][0] if names_m else None):
                self.v_end = off
            self.index[n] = (off, p.numel(), tuple(p.shape))
            off += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        if not names_m:
            self.v_end = off
        self.total = off
        self.order = [n for n, _ in names_v + names_m]
        self.p32 = torch.zeros(self.total, device=self.device, dtype=torch.float32)
        self.g32 = torch.zeros(self.total, device=self.device, dtype=torch.float32)
        self.p16 = torch.zeros(self.total, device=self.device, dtype=torch.bfloat16) if compute_dtype == torch.bfloat16 else None
        # lo half of the shadow PAIR (round 6): p16lo = bf16(p32 - p16), same offsets -- the B_lo operand of the forward products of
        # small stacks (EncoderStack.pair_w).  Kept by everything that keeps p16 (refresh_shadow, the fused BertAdam update and its riders).
        # Allocated when the first plan asks for it (ensure_lo: model.operand_pairs holds 'w'), never by default.
        self.p16lo = None
        self.operand_pairs = str(_ab.get("pairs"))       # '', 'x', 'w', 'xw' (UniVL.operand_pairs)
        self.params = {}
        with torch.no_grad():
            for n, p in names_v + names_m:
                o, k, shp = self.index[n]
                view = self.p32[o:o + k].view(shp)
                view.copy_(p.detach().to(self.device, torch.float32))
                p.data = view
                self.params[n] = p
        self.shadow_valid = False
        self.grad_version = 0        # bumped by every backward; pairs a clip measurement with the gradients it saw
        self._clip = None
        self._pending = None
        # per-tensor sums of squared gradients written by the weight-gradient GEMMs themselves (UnivlGemm.sumsq)
        self.seg_of = {n: i for i, n in enumerate(self.order)}
        self.sumsq = torch.zeros(len(self.order), device=self.device, dtype=torch.float32)
        # per-wave partial sums: <= 4 per 64x64 output tile of every matrix
        m_elems = self.total - self.v_end
        self.partials = torch.zeros(m_elems // 1024 + 8 * len(self.order) + 64, device=self.device, dtype=torch.float32)
        self.fused = None            # dict(version=grad_version, names=frozenset) once a backward produced them
        # Word-table rows that have EVER held a non-zero gradient / moment (uint8 per row, sticky): the fused BertAdam update takes
        # the weight-decay-only shortcut on chunks of rows that never did (UnivlAdam.row_flags, optim.hip) -- at most B*W of the
        # 30522 rows are touched per step, the table is 15 % of all parameters.  Valid from here on because g32 (and the moments of
        # any optimizer created later) start at zero; every event after which a row's g / m / v can be non-zero without having gone
        # through univl_rows_append marks ALL rows (mark_all_word_rows).
        self.word_ever = None
        if self.WORD in self.index and _ab.get("adam_lazy_rows"):
            self.word_ever = torch.zeros(self.index[self.WORD][2][0], dtype=torch.uint8, device=self.device)
        self.word_ever_all = False
        self._gviews = {}
        self.name_of = {id(p): n for n, p in self.params.items()}
        FLAT_REGISTRY.add(self)

    def is_atomic(self, name):
        return self.index[name][0] < self.v_end

    WORD = "bert.embeddings.word_embeddings.weight"
    WORD_ROWS_CAP = 8192

    def word_rows(self):
        """(list, meta) device buffers of the sparse word-table bookkeeping (univl_rows_zero / _append / _sumsq): the table
        rows written by the backward passes since the last clear."""
        if getattr(self, "_word_rows", None) is None:
            # created lazily by the first backward that uses the bookkeeping -- earlier backwards (a batch above WORD_ROWS_CAP, the
            # dense path) may have written any row of the table: start in the "every row counts as listed" state
            meta = torch.zeros(2, dtype=torch.int32, device=self.device)
            meta[1] = 1
            self._word_rows = (torch.zeros(self.WORD_ROWS_CAP, dtype=torch.int64, device=self.device), meta)
            self.word_rows_version = -1
        return self._word_rows

    def mark_all_word_rows(self):
        """Somebody wrote the word table's gradient (or its moments) without listing the rows: no row may take the shortcut."""
        if self.word_ever is not None and not self.word_ever_all:
            self.word_ever.fill_(1)
            self.word_ever_all = True

    def v_region_without_word_table(self):
        """Slices of g32 covering the atomic region except the word-embedding table."""
        o, k, _ = self.index[self.WORD]
        end = o + (k + _ALIGN - 1) // _ALIGN * _ALIGN
        return [t for t in (self.g32[:o], self.g32[end:self.v_end]) if t.numel() > 0]

    # ---- views
    def w32(self, name):
        o, k, shp = self.index[name]
        return self.p32[o:o + k].view(shp)

    def g(self, name):
        """Gradient view of a parameter (one cached tensor object per name: `p.grad is flat.g(name)` identifies our own
        gradient storage without touching data pointers)."""
        v = self._gviews.get(name)
        if v is None:
            o, k, shp = self.index[name]
            v = self._gviews[name] = self.g32[o:o + k].view(shp)
        return v

    def wop(self, name):
        """compute-type view of a weight (bf16 shadow or the fp32 master itself)."""
        o, k, shp = self.index[name]
        src = self.p16 if self.p16 is not None else self.p32
        return src[o:o + k].view(shp)

    def ensure_lo(self):
        """The lo half of the shadow pair exists from here on (615 MB -> 920 MB of shadow at 152 M parameters); filled from the fp32
        master now if the hi half is current, else by the refresh that is due anyway."""
        if self.p16lo is None and self.p16 is not None:
            self.p16lo = torch.zeros(self.total, device=self.device, dtype=torch.bfloat16)
            if self.shadow_valid:
                ops.cast_bf16_pair(self.p32, None, self.p16lo)
        return self.p16lo is not None

    def wlo(self, name):
        """lo half of a weight's shadow pair (None: no pairs)."""
        if self.p16lo is None:
            return None
        o, k, shp = self.index[name]
        return self.p16lo[o:o + k].view(shp)

    def wlo_fused(self, names):
        return None if self.p16lo is None else self._fused(self.p16lo, names)

    def _fused(self, buf, names):
        o0, _, shp0 = self.index[names[0]]
        rows, o = 0, o0
        for n in names:
            on, k, shp = self.index[n]
            assert on == o and shp[1:] == shp0[1:], "parameters %s are not contiguous in the flat buffer" % (names,)
            assert k % _ALIGN == 0
            o += k
            rows += shp[0]
        return buf[o0:o].view((rows,) + tuple(shp0[1:]))

    def wop_fused(self, names):
        return self._fused(self.p16 if self.p16 is not None else self.p32, names)

    def w32_fused(self, names):
        return self._fused(self.p32, names)

    def g_fused(self, names):
        return self._fused(self.g32, names)

    def refresh_shadow(self, force=False):
        if self.p16 is not None and (force or not self.shadow_valid):
            if getattr(self, "shard_reducer", None) is not None and not getattr(self, "master_complete", True):
                raise RuntimeError("FlatParams.refresh_shadow: the fp32 master weights are sharded over the ranks and this rank's copy of "
                                   "the other ranks' pieces is stale -- call model.consolidate_parameters() (a collective) first")
            if self.p16lo is not None:
                ops.cast_bf16_pair(self.p32, self.p16, self.p16lo)
            else:
                ops.cast_bf16(self.p32, self.p16)
        self.shadow_valid = True

    def attach_grads(self, used_names):
        """p.grad <- view of g32 for every parameter that receives a gradient in this configuration."""
        for n in used_names:
            p, gv = self.params[n], self.g(n)
            if p.grad is not gv:
                p.grad = gv


class GradState:
    """Book-keeping while a backward plan is built: the first weight-gradient GEMM that writes a matrix in a FRESH
    backward uses beta = 0 (no 600 MB memset, no read-modify-write); later writers of the same tensor (tied weights,
    a module that runs twice in one step) and every backward under gradient accumulation use beta = 1.  Tensors of the
    atomic region are zeroed by one memset when fresh and always accumulated into."""

    def __init__(self, flat, fresh, fuse_sumsq=False):
        self.flat, self.fresh, self.written = flat, fresh, set()
        self.fuse_sumsq, self.covered = bool(fuse_sumsq), set()
        self.slots, self.entries = 0, []             # partial-sum slots handed out; (segment, start, count) per tensor

    def sumsq_args(self, names, rows_per_tensor, cols):
        """Keyword arguments for the weight-gradient GEMM that writes `names` (one matrix, or the adjacent matrices of a
        fused projection, each rows_per_tensor x cols): have its epilogue store per-wave partial sums of squares.
        Only in configurations where every matrix has exactly one writer per backward (checked here)."""
        if isinstance(names, str):
            names = [names]
        if not self.fuse_sumsq or any(self.flat.is_atomic(n) for n in names) or rows_per_tensor % 128 != 0:
            return {}
        if any(n in self.covered for n in names):
            raise RuntimeError("fused gradient norms: %s has a second writer in this backward" % (names,))
        self.covered.update(names)
        stride = (rows_per_tensor // 64) * ((cols + 63) // 64) * 4          # slots per tensor with the smallest tile
        start = self.slots
        for t, n in enumerate(names):
            self.entries.append((self.flat.seg_of[n], start + t * stride, stride))
        self.slots += stride * len(names)
        if self.slots > self.flat.partials.numel():
            raise RuntimeError("fused gradient norms: partial-sum buffer too small")
        return dict(sumsq=self.flat.partials[start:], sumsq_rows=rows_per_tensor if len(names) > 1 else 0, sumsq_stride=stride)

    def acc(self, name):
        if self.flat.is_atomic(name):
            return True
        a = (not self.fresh) or (name in self.written)
        self.written.add(name)
        return a

    def finish(self, plan):
        """Zeroing of the partial sums goes to the front of the backward (caller), this fold to its end."""
        if not self.entries:
            return
        dev = self.flat.device
        seg, start, count = (torch.tensor(x, dtype=torch.int32, device=dev) for x in zip(*self.entries))
        out = self.flat.sumsq
        plan.add_callable(lambda: ops.sumsq_finish(self.flat.partials, seg, start, count, out))


class Riders:
    """The prepared BertAdam update that rides in ONE run of a plan (Plan.riders): its descriptor, the chunk range (first, count) of
    every key the run carries, and which (key, slot) launches have taken their part so far."""
    __slots__ = ("desc", "ref", "ranges", "max_blocks", "used", "nslots", "graphed")

    def __init__(self, desc, ranges, max_blocks=0):
        self.desc, self.ref, self.ranges, self.max_blocks, self.used = desc, C.byref(desc), dict(ranges), int(max_blocks), set()
        self.nslots = {}             # key -> over how many launches its range is dealt (known once one of them took its part)
        # None: the run enqueues its launches directly, `used` tells what has gone out.  Plan.run_graphed: a capture takes parts that no
        # kernel has applied yet and a replay applies parts nobody takes, so `used` tells nothing -- False while that run is under way
        # (what has gone out cannot be told), True once its last segment has been replayed (every range has).
        self.graphed = None

    def take(self, key, slot, nslots):
        """(first, count) of the chunks the launch that is slot `slot` of `nslots` for `key` carries now, or None: nothing rides under
        that key, or the slot has gone out -- a stack that runs twice in one forward (pretrain: clean and masked pass) carries once."""
        rng = self.ranges.get(key)
        if rng is None or (key, slot) in self.used:
            return None
        self.used.add((key, slot))
        self.nslots[key] = nslots
        lo = rng[0] + rng[1] * slot // nslots
        return lo, rng[0] + rng[1] * (slot + 1) // nslots - lo

    def signature(self):
        """What a capture of the carrying plan bakes in (UniVL._run_plan replays a graph only under the signature it was captured with)."""
        return bytes(self.desc), tuple(sorted(self.ranges.items())), self.max_blocks

    def pending(self):
        """[(key, first, count, partly)] of every range of this run: partly False, nothing of it has gone out; True, some slot has -- the
        slots are fractions only the plan knows, so which chunks did cannot be told from here -- unless all of them did: whole()
        (optimization.PendingUpdate.complete_after_failure).  A run through graphs: every key counts as partly sent."""
        sent = set(self.ranges) if self.graphed is not None else {key for key, _ in self.used}
        return [(key, c0, n, key in sent) for key, (c0, n) in self.ranges.items()]

    def whole(self, key):
        """Every slot of `key` has gone out: its range is applied."""
        if self.graphed is not None:
            return self.graphed
        n = self.nslots.get(key, 0)
        return n > 0 and all((key, s) in self.used for s in range(n))


class Op:
    """One entry of Plan.ops.  Every op has kind, name (the entry point's name) and stream; launch forms (the subclasses below) have fn
    and descs (their GEMM-family descriptors: Plan.descs[i] is the same list), and key / slot / nslots where they can carry optimizer
    chunks (key None: they carry none); "eager" / "pys" / "py" have fn, "record" / "wait" key, "dep" src and dst.  `was`: what stood at
    position 2 of the five-tuple an op used to be, kept for __getitem__ alone."""
    __slots__ = ("kind", "name", "stream", "fn", "descs", "key", "slot", "nslots", "src", "dst", "was")

    def __init__(self, kind, name, stream=0, fn=None, key=None, src=None, dst=None):
        self.kind, self.name, self.stream, self.fn, self.key, self.src, self.dst = kind, name, stream, fn, key, src, dst
        self.descs = self.slot = self.nslots = self.was = None

    def __getitem__(self, i):
        """op[0] .. op[4] of the former tuple, (kind, fn | key | src, payload | dst, name, stream): the tests of earlier commits read plans
        that way and must keep passing against this one.  Nothing in the package does; new readers use the fields."""
        a, b = (self.src, self.dst) if self.kind == "dep" else (self.key if self.fn is None else self.fn, self.was)
        return (self.kind, a, b, self.name, self.stream)[i]


class Launch(Op):
    """A launch form: how it is enqueued on a stream handle (enqueue -> rc; `riders`: Plan.riders of this run) and how Plan.launches
    replays it (replay -> (launch(handle) -> rc, descriptors)).  This one: an entry point called as fn(*args, handle), replayed as it ran."""
    __slots__ = ("args",)

    def __init__(self, kind, name, stream, descs, args, key=None, slot=0, nslots=1, entry=None):
        Op.__init__(self, kind, name, stream, getattr(_lib.lib(), entry or name), key)
        self.descs, self.args, self.slot, self.nslots = descs, args, int(slot), int(nslots)

    def enqueue(self, h, riders=None):
        return self.fn(*self.args, h)

    def counts_as(self, prefix):  # ("call2": univl_pool_pair_fwd / _bwd, in no replayed family)
        return self.kind != "call2" and self.name.startswith(prefix)

    def replay(self, carried):
        return self.enqueue, self.descs


class _Carrier(Launch):
    """A launch that does other work beside its dense contractions (optimizer chunks, a LayerNorm, the attention around a projection):
    replayed as the contractions alone.  `gemms`: where among args their descriptors sit.  A form's entry point (`entry`) takes (*args,
    *chunks, dry_run, stream): args as pack builds them from its descriptors, chunks only where it can carry some (`idle`: none ride)."""
    __slots__ = ()
    gemms, idle = slice(0, 1), ()

    def __init__(self, kind, stream, descs, args, key=None, slot=0, nslots=1):
        Launch.__init__(self, kind, self.entry, stream, descs, args, key, slot, nslots)

    def whole(self, h, chunks=None):
        """The launch with everything it carries but the chunks, or with `chunks`."""
        return self.fn(*self.args, *(chunks or self.idle), 0, h)

    def enqueue(self, h, riders=None):
        return self.whole(h, self.chunks(riders))

    @classmethod
    def accepts(cls, *descs):
        """Does the library carry this form for these descriptors (pack's arguments)?  The entry point's dry run: nothing is enqueued."""
        return getattr(_lib.lib(), cls.entry)(*cls.pack(*descs), *cls.idle, 1, None) == 0

    def chunks(self, riders):
        """(update, first, count, max_blocks) of the optimizer chunks this launch carries in this run, or None."""
        part = None if riders is None or self.key is None else riders.take(self.key, self.slot, self.nslots)
        return part and (riders.ref, part[0], part[1], riders.max_blocks)

    def dense(self, h):
        """The dense contraction alone: what the launch falls back to without the work it carries, and what it is replayed as."""
        g = [a for a in self.args[self.gemms] if a is not None]
        return _lib.lib().univl_gemm(g[0], h) if len(g) == 1 else _lib.lib().univl_gemm_pair(g[0], g[1], 0, h)

    def replay(self, carried):    # (optimizer chunks never replay: they would change the parameters)
        return self.dense, self.descs


class _Rider(_Carrier):           # (univl_gemm_rider takes no dry_run: fits is its probe; without chunks the plain product goes out)
    __slots__ = ()
    entry = "univl_gemm_rider"
    fits = staticmethod(lambda desc: _lib.lib().univl_gemm_rider_fits(C.byref(desc)) == 1)

    def enqueue(self, h, riders=None):
        ad = self.chunks(riders)
        return self.dense(h) if ad is None else self.fn(*self.args, *ad, h)


class _Pair(_Carrier):            # (a dgrad product and the weight-gradient product fed by the same upstream gradient: replayed as it ran)
    __slots__ = ()
    entry, gemms = "univl_gemm_pair", slice(0, 2)
    pack = staticmethod(lambda dgrad, wgrad: (C.byref(dgrad), C.byref(wgrad)))


class _LnFold(_Carrier):
    """... that finishes the LayerNorm `ln` behind its product: whole(h) is the launch with it and without chunks; `ln_entry` runs the
    LayerNorm alone, on the argument that follows the products."""
    __slots__ = ("ln",)

    def enqueue(self, h, riders=None):
        ad = self.chunks(riders)
        rc = self.whole(h, ad)
        if rc == _lib.EUNSUPPORTED:      # deterministic mode (or a shape the fold does not carry): the two launches
            rc = self.dense(h) if ad is None else _lib.lib().univl_gemm_rider(self.args[0], *ad, h)
            rc = rc or getattr(_lib.lib(), self.ln_entry)(self.args[self.gemms.stop], h)
        return rc

    def replay(self, carried):    # carried: with its LayerNorm, whose descriptor then ends the list
        return (self.whole, self.descs + [self.ln]) if carried else (self.dense, self.descs)


class _GemmLn(_LnFold):
    __slots__ = ()
    entry, ln_entry, idle = "univl_gemm_ln", "univl_layernorm_fwd", (None, 0, 0, 0)
    pack = staticmethod(lambda desc, ln_desc, counters: (C.byref(desc), C.byref(ln_desc), C.c_void_p(counters.data_ptr())))


class _PairLn(_LnFold):
    __slots__ = ()
    entry, ln_entry, gemms = "univl_gemm_pair_ln", "univl_layernorm_bwd", slice(0, 2)
    pack = staticmethod(lambda dgrad, wgrad, ln_desc, counters: (C.byref(dgrad), C.byref(wgrad), C.byref(ln_desc), C.c_void_p(counters.data_ptr())))


class _FusedAttn(_Carrier):
    """... the fused attention launches: the dense contractions inside them belong to the GEMM family, and to no other, and are replayed
    the way they ran before the fused launches existed (the family's accounting)."""
    __slots__ = ()

    def counts_as(self, prefix):
        return prefix == "univl_gemm"


class _AttnFwdFused(_FusedAttn):
    __slots__ = ("attn",)
    entry, gemms, idle = "univl_attention_fwd_fused", slice(1, 2), (None, 0, 0, 0)
    pack = staticmethod(lambda attn, qkv: (C.byref(attn), C.byref(qkv)))


class _AttnBwdFused(_FusedAttn):  # (owgrad: the attention-output weight gradient that rides, or None)
    __slots__ = ()
    entry, gemms = "univl_attention_bwd_fused", slice(1, 3)
    pack = staticmethod(lambda attn, odgrad, owgrad: (C.byref(attn), C.byref(odgrad), owgrad if owgrad is None else C.byref(owgrad)))


class Plan:
    """A static list of kernel enqueues over a small set of HIP streams.

    Stream 0 is whatever stream is current when run() is called (the capture stream under hipGraph capture); the
    others are side streams created once per plan.  fork(a, b) makes b wait for everything enqueued on a so far,
    join(a, b) is the same edge written from the consumer's side -- both are event record/wait pairs, which a
    hipGraph capture turns into plain dependency edges, so independent chains (weight-gradient GEMMs, the text and
    the video encoder) run concurrently on the 256 CUs instead of queueing behind the critical path."""

    def __init__(self):
        self.ops = []                # Op records, in enqueue order
        self.keep = []
        self.descs = {}              # op index -> the C descriptors of that launch (measurement / introspection)
        self.external = {}           # key -> event recorded by somebody else (see wait_point)
        self._side = {}
        self._segments = None        # captured segments of run_graphed() under the rider signature _rider_sig ...
        self._rider_sig = None
        self._seg_cache = {}         # ... and those of other signatures (select_segments)
        self.rider_keys = set()      # chunk-group keys this plan can carry beside its forward products (add_gemm_rider)
        self.riders = None           # set for the duration of one run: the Riders that run carries (None: nothing rides)

    def _launch(self, op, keep, was):
        self.keep += keep
        op.was = was
        self.descs[len(self.ops)] = op.descs
        if op.key is not None:
            self.rider_keys.add(op.key)
        self.ops.append(op)
        return op

    def add_gemm_rider(self, desc, key, slot, nslots, stream=0):
        """A forward product that, while self.riders names a chunk range for `key`, also carries
        the slot-th of nslots parts of that range of a prepared BertAdam update (univl_gemm_rider); otherwise a plain univl_gemm."""
        self._launch(_Rider("rider", stream, [desc], (C.byref(desc),), key, slot, nslots), [desc], (desc, key, int(slot), int(nslots)))

    def add_gemm_ln(self, desc, ln_desc, counters, key=None, slot=0, nslots=1, stream=0):
        """A forward product AND the LayerNorm that consumes its fp32 output in one launch (univl_gemm_ln: the last workgroups to
        contribute to a 64-row block normalise it); with `key` it also carries optimizer chunks like add_gemm_rider.  `counters`: the
        call site's int32 arrival counters (zeroed at allocation, left zero by every launch)."""
        was = (desc, ln_desc, counters, key, int(slot), int(nslots))
        self._launch(_GemmLn("gemm_ln", stream, [desc], _GemmLn.pack(*was[:3]), key, slot, nslots), was[:3], was).ln = ln_desc

    def add(self, fn_name, desc, stream=0):
        ref = C.byref(desc)
        self._launch(Launch("call", fn_name, stream, [desc], (ref,)), [desc], ref)

    def add_pair_call(self, fn_name, da, db, stream=0):
        """An entry point that takes two descriptors (univl_pool_pair_fwd / _bwd)."""
        self._launch(Launch("call2", fn_name, stream, [da, db], (C.byref(da), C.byref(db))), [da, db], (da, db))

    def add_gemm_group(self, descs, stream=0, max_blocks=0):
        """Independent GEMMs with the same operand layouts as ONE launch (univl_gemm_group), in chunks of GEMM_GROUP_MAX.
        max_blocks > 0: at most that many workgroups (the kernel walks its tiles)."""
        if not _ab.get("group_wgrad"):           # A/B: one launch per member
            for d in descs:
                self.add("univl_gemm", d, stream)
            return
        for i in range(0, len(descs), _lib.GEMM_GROUP_MAX):
            chunk = descs[i:i + _lib.GEMM_GROUP_MAX]
            arr = (_lib.Gemm * len(chunk))(*chunk)
            args = (arr, len(chunk), int(max_blocks))
            self._launch(Launch("group", "univl_gemm_group", stream, list(chunk), args, entry="univl_gemm_group_limited"), [arr], args)

    def add_gemm_pair(self, dgrad, wgrad, stream=0):
        """A dgrad product and the weight-gradient product fed by the same upstream gradient as
        ONE launch (univl_gemm_pair) -- the weight-gradient tiles fill the compute units the latency-bound dgrad leaves idle."""
        arr = (_lib.Gemm * 2)(dgrad, wgrad)
        self._launch(_Pair("pair", stream, [dgrad, wgrad], _Pair.pack(arr[0], arr[1])), [arr], arr)

    def add_attn_fwd_fused(self, attn, qkv, key=None, slot=0, nslots=1, stream=0):
        """The attention forward with the q | k | v projection computed inside the launch (univl_attention_fwd_fused); with `key` it
        also carries optimizer chunks like add_gemm_rider."""
        self._launch(_AttnFwdFused("attn_fwd_fused", stream, [qkv], _AttnFwdFused.pack(attn, qkv), key, slot, nslots), [attn, qkv],
                     (attn, qkv, key, int(slot), int(nslots))).attn = attn

    def add_attn_bwd_fused(self, attn, odgrad, owgrad, stream=0):
        """The attention backward with the attention-output dgrad that feeds it computed inside the launch, the weight gradient of
        that projection riding as extra workgroups (univl_attention_bwd_fused; owgrad may be None)."""
        was, descs = (attn, odgrad, owgrad), [odgrad] + ([owgrad] if owgrad is not None else [])
        self._launch(_AttnBwdFused("attn_fused", stream, descs, _AttnBwdFused.pack(*was)), list(was), was)

    def add_gemm_pair_ln(self, dgrad, wgrad, ln_desc, counters, stream=0):
        """add_gemm_pair with the LayerNorm BACKWARD that consumes the dgrad's fp32 output finished inside the launch
        (univl_gemm_pair_ln); falls back to the two launches at run time where the library refuses (deterministic mode)."""
        arr = (_lib.Gemm * 2)(dgrad, wgrad)
        args, was = _PairLn.pack(arr[0], arr[1], ln_desc, counters), (arr, ln_desc, counters)
        self._launch(_PairLn("pair_ln", stream, [dgrad, wgrad], args), list(was), was).ln = ln_desc

    def add_zeros(self, tensors, stream=0):
        """Clear several buffers with one launch (univl_zero_many)."""
        ts = [t for t in tensors if t is not None and t.numel() > 0]
        if ts:
            self.add_callable(lambda: ops.zero_many(ts), stream)

    def add_callable(self, f, stream=0, eager=False, with_streams=False):
        """eager=True marks host-driven work that must never be captured into a hipGraph (collectives of torch's process group):
        run() treats it like any callable, run_graphed() replays the captured kernels on either side of it and calls it
        in between, on the calling stream.  with_streams=True (capturable): f is called as f(streams) with every stream the plan
        has enqueued work on so far (the calling stream first) -- a gradient exchange on a communication stream of its own waits for
        exactly those, without joining them into the main chain."""
        kind = "eager" if eager else ("pys" if with_streams else "py")
        self.ops.append(Op(kind, getattr(f, "__name__", "callable"), stream, fn=f))

    def wait_point(self, key, stream=0):
        """If an event is registered under `key` in self.external when the plan runs, `stream` waits for it; otherwise a
        no-op.  The pipelined training step (univl_amd.graphed) applies the previous step's BertAdam update layer by layer
        on its own stream and registers one event per layer; the forward plan waits for a layer's parameters only where it
        first reads them."""
        self.ops.append(Op("wait", "wait", stream, key=key))

    def record(self, key, stream=0):
        """Mark the work enqueued on `stream` so far; a later wait_point(key, other_stream) waits for exactly that much
        (fork / join always wait for everything enqueued on the source up to the moment of the wait)."""
        self.ops.append(Op("record", "record", stream, key=key))

    def fork(self, src, dst):
        """dst waits for all work enqueued on src so far."""
        if src != dst:
            self.ops.append(Op("dep", "dep", 0, src=src, dst=dst))

    def join(self, src, dst):
        self.fork(src, dst)

    def _stream(self, idx, cur):
        if idx == 0:
            return cur
        st = self._side.get(idx)
        if st is None or st.device != cur.device:
            st = torch.cuda.Stream(device=cur.device)
            self._side[idx] = st
        return st

    def _run_ops(self, ops_, cur, forked=None):
        handles, events, riders = {}, {}, self.riders
        forked = set() if forked is None else set(forked)       # side-stream indices ordered behind `cur` in this run
        for op in ops_:
            kind, sidx = op.kind, op.stream
            if op.descs is not None:                            # a launch form
                h = handles.get(sidx)
                if h is None:
                    h = handles[sidx] = C.c_void_p(self._stream(sidx, cur).cuda_stream)
                rc = op.enqueue(h, riders)
                if rc != 0:
                    if riders is not None and op.key is not None:
                        riders.nslots[op.key] = 0           # whether a part this launch took went out cannot be told: never whole()
                    _lib.check(rc, op.name)
            elif kind == "record":
                ev = torch.cuda.Event()
                ev.record(self._stream(sidx, cur))
                events[op.key] = ev
            elif kind == "wait":
                ev = events.get(op.key)
                if ev is None and self.external:
                    ev = self.external.get(op.key)
                if ev is not None:
                    self._stream(sidx, cur).wait_event(ev)
            elif kind == "eager":
                for sd in self._side.values():             # host-driven exchange point: everything planned so far
                    if sd.device == cur.device:
                        cur.wait_stream(sd)
                op.fn()
            elif kind == "pys":
                # only the side streams THIS run has forked so far (the last "dep" into a stream orders it behind the calling
                # stream; under capture a stream that has not joined the capture yet must not be waited for)
                op.fn([cur] + [self._stream(i, cur) for i in sorted(forked)])
            elif kind == "py":
                if sidx == 0:
                    op.fn()
                else:
                    with torch.cuda.stream(self._stream(sidx, cur)):
                        op.fn()
            else:
                self._stream(op.dst, cur).wait_stream(self._stream(op.src, cur))
                if op.dst != 0:
                    forked.add(op.dst)

    def run(self, upto=None):
        self._run_ops(self.ops if upto is None else self.ops[:upto], torch.cuda.current_stream())

    def segments(self):
        """[("graph", ops) | ("eager", op), ...]: maximal runs of capturable ops between eager ops."""
        out, cur = [], []
        for op in self.ops:
            if op.kind == "eager":
                if cur:
                    out.append(("graph", cur))
                    cur = []
                out.append(("eager", op))
            else:
                cur.append(op)
        if cur:
            out.append(("graph", cur))
        return out

    def select_segments(self, sig, keep):
        """Make the captured segments of rider signature `sig` (Riders.signature(), None: nothing rides) the ones run_graphed() replays;
        True: there are none, run_graphed() is going to capture.  A capture bakes in the riding update's descriptor and chunk ranges, so
        segments are kept PER signature: under gradient accumulation the forward after step() carries riders and the following ones do
        not -- both are captured once and replayed, not re-captured at every transition.  At most `keep` signatures stay alive, this
        one included; the one unused longest goes first."""
        if sig != self._rider_sig:
            segs = self._seg_cache.pop(sig, None)
            if self._segments is not None:
                self._seg_cache[self._rider_sig] = self._segments
                while len(self._seg_cache) >= keep:
                    self._seg_cache.pop(next(iter(self._seg_cache)))
            self._segments, self._rider_sig = segs, sig
        return self._segments is None

    def run_graphed(self):
        """Replay the plan as hipGraphs: every run of kernels between two eager ops is captured once (on first use)
        and replayed afterwards; eager ops (collectives) are issued from the host between the replays, on the calling
        stream.  A captured segment must be self-contained, so side streams are forked from the capture stream at
        its start and joined back at its end -- a cut inside a forked region costs one extra join, never correctness."""
        if self._segments is None:
            segs = []
            for kind, payload in self.segments():
                if kind == "eager":
                    segs.append(["eager", payload, None])
                else:
                    sides = sorted({op.stream for op in payload if op.kind != "dep" and op.stream != 0}
                                   | {x for op in payload if op.kind == "dep" for x in (op.src, op.dst) if x != 0})
                    segs.append(["graph", payload, None, sides])
            self._segments = segs
        if self.riders is not None:
            self.riders.graphed = False      # until the last replay below: a failure in between cannot tell what has gone out
        for seg in self._segments:
            if seg[0] == "eager":
                seg[1].fn()
                continue
            if seg[2] is None:
                g = torch.cuda.CUDAGraph()
                # thread_local: RCCL's watchdog thread may query events of in-flight collectives during the capture
                with no_gc(), torch.cuda.graph(g, capture_error_mode="thread_local"):
                    cur = torch.cuda.current_stream()
                    sides = [self._stream(i, cur) for i in seg[3]]
                    for sd in sides:
                        sd.wait_stream(cur)
                    self._run_ops(seg[1], cur, forked=seg[3])
                    for sd in sides:
                        cur.wait_stream(sd)
                seg[2] = g
            seg[2].replay()
        if self.riders is not None:
            self.riders.graphed = True

    def launches(self, prefix, carried=False):
        """[(launch(stream_handle), [descriptors])] for every planned launch whose entry point starts with `prefix`, in plan
        order -- bench.py replays one kernel family alone to time it with HIP events.  A product that CARRIES other work in the step
        (optimizer chunks: add_gemm_rider; the LayerNorm behind it: add_gemm_ln / add_gemm_pair_ln) is replayed without it by
        default -- the dense contraction alone, the quantity rounds 1-3 report -- and with its LayerNorm when carried=True (the
        descriptor list then ends with that LayerNorm descriptor; optimizer chunks never replay: they would change the parameters).
        The fused attention launches count under "univl_gemm" only, as the dense contractions inside them."""
        return [op.replay(carried) for op in self.ops if op.descs is not None and op.counts_as(prefix)]

    @property
    def calls(self):
        return self.ops

    def __len__(self):
        return len(self.ops)


def _gemm_desc(dt, A, lda, B, ldb, M, N, K, *, trans_a=0, trans_b=0, out32=None, out16=None, ldc=0, bias=None,
               residual=None, ldr=0, aux=None, ldaux=0, gelu=None, accumulate=False, dbias=None, ksplit=1, tile=0,
               sumsq=None, sumsq_rows=0, sumsq_stride=0, nt_out=False, stages=0, waves=0, aux_f32=False, a_lo=None, b_lo=None,
               out16_lo=None):
    """a_lo / b_lo / out16_lo: lo halves of operand pairs (UnivlGemm.A_lo ...; same layout as A / B / out16), or None."""
    d = _lib.Gemm()
    d.dtype, d.trans_a, d.trans_b, d.M, d.N, d.K = dt, trans_a, trans_b, M, N, K
    d.A, d.lda, d.B, d.ldb = A.data_ptr(), lda, B.data_ptr(), ldb
    d.C32 = out32.data_ptr() if out32 is not None else None
    d.C16 = out16.data_ptr() if out16 is not None else None
    d.ldc = ldc
    d.bias = bias.data_ptr() if bias is not None else None
    d.R, d.ldr = (residual.data_ptr() if residual is not None else None), ldr
    d.aux, d.ldaux = (aux.data_ptr() if aux is not None else None), ldaux
    d.dbias = dbias.data_ptr() if dbias is not None else None
    d.alpha = 1.0
    flags = _lib.GEMM_DBIAS_ATOMIC if dbias is not None else 0
    if accumulate:
        flags |= _lib.GEMM_ACCUM
    elif nt_out:
        flags |= _lib.GEMM_NT_OUT
    if gelu == "fwd":
        flags |= _lib.GEMM_GELU_FWD
    elif gelu == "bwd":
        flags |= _lib.GEMM_GELU_BWD
    if aux_f32:
        flags |= _lib.GEMM_AUX_F32
    d.flags, d.ksplit, d.tile = flags, ksplit, tile
    d.sumsq, d.sumsq_rows, d.sumsq_stride = (sumsq.data_ptr() if sumsq is not None else None), sumsq_rows, sumsq_stride
    d.stages, d.waves = stages, waves
    d.A_lo = a_lo.data_ptr() if a_lo is not None else None
    d.B_lo = b_lo.data_ptr() if b_lo is not None else None
    d.C16_lo = out16_lo.data_ptr() if out16_lo is not None else None
    return d


class _SiteCounter:
    """Distinct dropout stream offsets per call site."""

    def __init__(self):
        self.n = 0

    def next(self):
        self.n += 1
        return self.n << 40


class EncoderStack:
    """BertEncoder / VisualEncoder / CrossEncoder (module_bert.py:253-281 and copies): L post-LN transformer
    layers over T = B*S tokens.  Builds forward and backward plans over a persistent workspace."""

    H, NH, I = 768, 12, 3072

    def __init__(self, flat, prefix, n_layers, B, S, key_mask, p_drop, seed_dev, sites, splitk=True, s_main=0, s_side=1):
        """(Measured and removed, numbers in DESIGN.md section 8: a layer's weight gradients on the OTHER stack's stream
        (UNIVL_WGRAD_OFFLOAD), "background" weight gradients capped at n workgroups on two alternating side streams
        (UNIVL_WGRAD_BLOCKS: correct when enqueued directly, crashes hipStreamEndCapture on ROCm 7.0.2), non-temporal stores of
        fresh weight gradients (UNIVL_WGRAD_NT), bias-gradient column sums as launches of their own (UNIVL_DBIAS_COLSUM_MIN,
        UNIVL_COLSUM_ON_CHAIN) -- since round 2 every weight gradient rides with its dgrad or sits in the layer's grouped launch.)"""
        self.flat, self.prefix, self.L, self.B, self.S = flat, prefix, n_layers, B, S
        self.sm, self.ss = s_main, s_side
        # Every weight-gradient GEMM rides in the launch of the dgrad GEMM that consumes the same upstream gradient
        # (Plan.add_gemm_pair) instead of the layer's grouped launch at the end of the chain: the grouped launch was the longest
        # node of the backward chain (29 of ~100 us per layer at 4 pairs) although nothing downstream waits for it, and the dgrad
        # kernels it now shares a launch with leave most compute units idle.  Measured 2.85 vs 3.11 ms per step at 4 pairs
        # (profiles/r02h_ab_wgrad_ride.txt).  bf16, 64 x 64 tiles only -- the C side refuses other pairs (univl_gemm_pair dry run)
        # and those weight gradients stay in the grouped launch.  UNIVL_WGRAD_RIDE=0: the grouped launch for all of them.
        # Round 5: from 1536 tokens on (multiples of 256, bf16) NO weight gradient rides -- all four go into the layer's grouped launch,
        # which the C side runs on the 256 x 256 8-phase body (csrc/gemm256.h), and every dgrad is a launch of its own on the tile
        # `choose` picks for it.  The pair launches were built for a few hundred tokens; at 3072 the QKV / FFN1 pairs (square 64 x 64
        # dgrad body walking a 2304 / 3072-deep contraction + 128 x 64 weight-gradient tiles) ran 112 us each, 36 of them per step = 4.0
        # of the 9.2 ms of the 64-pair step (profiles/r05f_bench_b64_kernel_stats.csv), against ~32 + ~40 us for the two dgrads alone
        # and 68 us for the layer's whole group.  g256=0 (univl_amd/_ab.py): the former plans.
        self.g256 = flat.compute_dtype == torch.bfloat16 and bool(_ab.get("g256")) and (B * S) % 256 == 0 and B * S >= _ab.get("g256_min_rows")
        self.ride = bool(_ab.get("wgrad_ride")) and flat.compute_dtype == torch.bfloat16 and not self.g256
        # The forward products of layer l can carry the BertAdam chunks of layer l + 1 (Plan.add_gemm_rider): switched on per model by
        # graphed.GraphedTrainStep(pipeline_optimizer=True) (flat.adam_ride), or for every model by UNIVL_ADAM_RIDE=1.
        # All passes of a stack through its layers in one forward (text / video: clean + masked pass; cross: up to three runs) are
        # enqueued one after the other on ONE stream, so a layer's update (carried by the FIRST pass through the layer before it)
        # is complete before anybody reads the layer.
        self.adam_ride = (getattr(flat, "adam_ride", False)
                          and flat.compute_dtype == torch.bfloat16 and prefix in ("bert", "visual", "cross"))
        self.tail_key = None         # chunk group carried by the products of the LAST layer (build_forward)
        # UNIVL_PROBE_SKIP=<prefix> (measurement only, scripts/probe_branches.py): this stack emits NO layer kernels, forward or
        # backward -- what the step costs without one of its two encoder branches (results are meaningless)
        self.probe_skip = _ab.get("probe_skip") == prefix
        # UNIVL_PROBE_NO_LN=fwd|bwd|both (measurement only): the encoder layers' LayerNorm launches are left out of the plan -- the step
        # time then bounds from above what ANY fusion of those nodes into their neighbours could save (results are meaningless)
        self.probe_no_ln = _ab.get("probe_no_ln")
        # (Round 4, measured and removed: the video stack's first layer updated by a launch on the video stack's own stream instead of in
        # front of the whole forward -- 2.391 / 2.391 / 2.427 vs 2.392 / 2.396 / 2.397 ms per step, profiles/r04f_ab_update_slot.txt: the
        # prologue launches are HBM streams, two of them side by side each run at half speed.)
        self.T = B * S
        # K8 / K10: the post-product LayerNorms of the forward finished inside the product's launch (Plan.add_gemm_ln, gemm.hip: ln_fold)
        # up to 640 tokens (round 6; 512 before: 576 tokens -2.6 %, 624 -1.7 %, 672 +-0, 768 +0.5 %, profiles/r06u_ab_fold_768*.txt) -- where a layer is a
        # chain of latency-bound launches and one kernel boundary per LayerNorm is worth more than
        # the fold's tail (three dependent round trips to the coherence point: atomics done, arrival counter, row loads).  Measured per
        # step, fold vs two launches (profiles/r04p_ab_ln_fold.txt, r04q_ab_ln_fold_sizes.txt): 192 tokens 2.271 vs 2.333 ms (-2.6 %),
        # 384: 2.780 vs 2.829 (-1.7 %), 576: 3.144 vs 3.148, 768: 3.469 vs 3.415 (+1.6 %); FT-Align 3.193 vs 3.318 (-3.8 %).
        # UNIVL_LN_FOLD=0: two launches (A/B).  Deterministic mode falls back to the two launches (the C side refuses).
        self.ln_fold = (flat.compute_dtype == torch.bfloat16 and B * S <= int(_ab.get("ln_fold_max_rows")) and bool(_ab.get("ln_fold"))
                        and prefix in ("bert", "visual", "cross"))
        self.key_mask = key_mask            # int64 [B,S] device tensor (static buffer)
        self.p = float(p_drop)
        self.seed_dev = seed_dev
        dev, T, H, I = flat.device, self.T, self.H, self.I
        ct = flat.compute_dtype
        self.bf = ct == torch.bfloat16
        f32 = torch.float32
        e = _workspace(dev)
        self.layers = []
        # Round 6 -- operand PAIRS in the forward products.  A bf16 MFMA operand carries 8 mantissa bits; at a few
        # hundred tokens the matrix pipe is < 10 % busy, so the forward products of small stacks take their activation operand (pair_x)
        # and / or their weight operand (pair_w) as hi + lo pairs of bf16 -- 16 mantissa bits -- and walk the contraction once per term
        # (x.W, x.W_lo, x_lo.W: UnivlGemm.A_lo / B_lo).  Every producer of such an activation writes the lo half beside the hi half
        # (LayerNorm / fold out16_lo, attention out_lo, the FFN1 epilogue's C16_lo); the backward reads the hi halves only, as before.
        # What it buys: the global gradient error against the reference's fp32 gradients 1.04e-2 -> (measured) at the benchmark's
        # configuration (profiles/r06_emul_bf16_*.txt: the emulated split of that error by rounding class).
        pr = str(getattr(flat, "operand_pairs", "")) if (self.bf and T <= int(_ab.get("pairs_max_rows")) and prefix in ("bert", "visual", "cross")) else ""
        self.pair_x = "x" in pr
        self.pair_w = "w" in pr and flat.ensure_lo()
        # A/B measurement (gelu_pre_f32=1): the saved FFN1 pre-activation in fp32 instead of bf16
        self.u_f32 = self.bf and bool(_ab.get("gelu_pre_f32"))
        # fp32 GEMM outputs that may be produced by split-K atomics live in two arenas zeroed ONCE per pass
        self.yarena = e(n_layers, 2, T, H)
        self.garena = e(n_layers, 2, T, H)
        self.ln_ctr = torch.zeros(n_layers, 2, 2 * ((T + 63) // 64), dtype=torch.int32, device=dev) if self.ln_fold else None   # arrival counters of the folds (every launch leaves them zero)
        # ... and the backward twin (Plan.add_gemm_pair_ln: the LayerNorm backward behind the FFN1 / QKV dgrad, square pair form: < 384 tokens).
        # Measured (profiles/r04r_ab_ln_fold_bwd.txt, three interleaved pairs at 4 pairs): 2.231 vs 2.260 ms per step (-1.3 %; no fold at
        # all: 2.357), 288 tokens 2.656 vs 2.665, FT-Align 3.144 vs 3.184, pretrain 9.66 vs 9.75.  UNIVL_LN_FOLD_BWD=0: two launches (A/B).
        # Round 5: the rectangular pair form (384+ tokens) carries it too (gemm_pair_kernel<true, 2, true>), up to 512 tokens where the
        # forward folds stop as well: 384 tokens 2.66 / 2.64 vs 2.69 / 2.68 ms per step (-1.3 %), 480 tokens 2.88 / 2.91 vs 2.93 / 2.93,
        # caption 5.164 / 5.168 vs 5.167 / 5.218, pretrain 9.31 / 9.31 vs 9.28 / 9.25 (profiles/r05x_ab_fold_bwd_rect.txt).
        self.ln_fold_bwd = self.ln_fold and T <= int(_ab.get("ln_fold_bwd_max")) and bool(_ab.get("ln_fold_bwd"))
        self.ln_ctr_b = torch.zeros(n_layers, 2, 2 * ((T + 63) // 64), dtype=torch.int32, device=dev) if self.ln_fold_bwd else None
        for l in range(n_layers):
            ws = dict(qkv=e(T, 3 * H, dtype=ct), lse=e(B, self.NH, S), ctx=e(T, H, dtype=ct),
                      y1=self.yarena[l, 0], st1=e(T, 2), a32=e(T, H), u=e(T, I, dtype=f32 if self.u_f32 else ct), f=e(T, I, dtype=ct),
                      y2=self.yarena[l, 1], st2=e(T, 2), o32=e(T, H))
            ws["a16"] = e(T, H, dtype=ct) if self.bf else ws["a32"]
            ws["o16"] = e(T, H, dtype=ct) if self.bf else ws["o32"]
            for k, cols in (("ctx", H), ("a16", H), ("f", I), ("o16", H)):        # lo halves of the activation pairs
                ws[k + "_lo"] = e(T, cols, dtype=ct) if self.pair_x else None
            ws["off"] = [sites.next() for _ in range(3)]     # attention probs, self-output, output dropout
            self.layers.append(ws)
        # backward scratch shared by all layers
        self.gbuf = e(T, H)
        self.dctx = e(T, H, dtype=ct)
        # operands of the weight-gradient GEMMs: dxd = grad wrt the FFN2 output, dxd2 = grad wrt the attention-output
        # projection (separate buffers: the four wgrads of a layer may be one grouped launch), du, dqkv
        self.scr = dict(dxd=e(T, H, dtype=ct), dxd2=e(T, H, dtype=ct), du=e(T, I, dtype=ct), dqkv=e(T, 3 * H, dtype=ct))
        # split-K of the products with H-wide outputs (N = 768: attention output, FFN2, and the dgrads of QKV / FFN1):
        #   * below 128 output tiles (a few hundred tokens) every one of them is split into ~384-deep slices -- the grid would not fill
        #     the chip otherwise (UNIVL_SPLITK_TILES / _LEN / _MAXWG, measured in rounds 1-3);
        #   * round 4, 128 .. 255 tiles (16 .. 28 pairs x 48 tokens; at 32 pairs it loses: 5.80 vs 5.59 ms), bf16: only the DEEP contractions (K = 2304, 3072) into three
        #     slices.  The phase trace at 768 tokens (profiles/r04c_trace_gemm_768_variants.txt): the unsplit products run 144
        #     workgroups through 18 - 24 dependent K steps (FFN2 forward 22.4 us -> 17.6 with three slices; the dgrad halves of the
        #     FFN1 / QKV pair launches 23 / 17 us of K loop alone); K = 768 stays whole.  Round 3 had found NO gain from splitting at
        #     this size (3.79 / 3.86 vs 3.69 / 3.71 ms per step) -- with the 64 x 64 pair launches of that round the extra dgrad
        #     workgroups pushed the weight-gradient tiles into a third round; the rectangular pair form (gemm.hip) fits them in one.
        self.tiles = ((T + 63) // 64) * (H // 64)
        # UNIVL_SPLITK_TILES: split the contraction of the N = 768 products while the 64 x 64 output grid has fewer tiles than this
        self.splitk = splitk and self.tiles < _ab.get("splitk_tiles")
        self.splitk_mid = (splitk and not self.splitk and self.bf and self.tiles < _ab.get("splitk_mid_tiles")
                           and bool(_ab.get("splitk_mid")))
        self.ks_h = self.ksplit_for(H) if self.splitk else 1
        self.any_split = self.splitk or self.splitk_mid
        # the zero-once arenas are needed wherever contributions arrive as fp32 atomics: split products, and every product a LayerNorm
        # fold rides on (univl_gemm_ln / univl_gemm_pair_ln force atomics also for unsplit products -- with splitk_tiles=0 the fold would
        # otherwise add onto the previous step's output)
        self.zero_y = self.any_split or self.ln_fold
        self.zero_g = self.any_split or self.ln_fold_bwd

    def ksplit_for(self, K, dgrad=False, site=None):
        if self.splitk_mid:
            # round 6 (profiles/r06k_ab_splitk_mid.txt, r06l_ab_splitk_mid_tiles.txt): three slices up to 160 tiles (16 pairs: 3.26 vs 3.29 ms
            # with two), two beyond (20 pairs 3.575 vs 3.626, 24 pairs 3.94 vs 4.05, 28 pairs 4.49 vs 4.60); K = 768 stays whole
            deep = int(_ab.get("splitk_mid_ks")) if self.tiles <= 160 else int(_ab.get("splitk_mid_ks_big"))
            return deep if K >= 2304 else int(_ab.get("splitk_mid_ks_768"))
        if not self.splitk:
            return 1
        if site is not None and _ab.get("ks_" + site):       # A/B: explicit slice count of one product of the layer
            return int(_ab.get("ks_" + site))
        tgt = _ab.get("splitk_target_wg") if self.tiles <= 48 else _ab.get("splitk_target_wg_big")
        if tgt:
            # Round 6: as many slices as bring tiles x slices to ~`tgt` workgroups, each at least 256 deep.  The rule of rounds 1-5
            # (384-deep slices, tiles x slices <= 512) dates from before the pair launches and the folds: at 192 tokens it made 288
            # workgroups of every K = 3072 product -- with its 288 weight-gradient tiles and 8 column-sum roles the FFN1 pair launch then
            # needs 584 resident slots of 512, i.e. a second round (phase trace, profiles/r06c_trace_gemm_192_weights_cold.txt: the
            # dgrad half is done after 11.6 us, the launch after 17.9).  Measured per step, alternating on one box
            # (profiles/r06h_ab_target_wg.txt, r06i_ab_target_wg2.txt): 4 pairs 2.210 -> 2.144 ms (-3.0 %) at 180; 8 pairs 2.652 -> 2.575
            # (-2.9 %) at 252 - 288; 10 pairs -1.6 %; FT-Align -2.6 %; pretrain 9.37 -> 9.03 (-3.4 %); caption -0.8 %; 12 pairs +-0.
            return max(1, min(int(tgt / self.tiles + 0.5), K // 256))
        per = _ab.get("splitk_len")
        ks = max(1, (K + per - 1) // per)
        cap = _ab.get("splitk_maxwg")
        if dgrad and _ab.get("splitk_dgrad_maxwg"):
            cap = min(cap, _ab.get("splitk_dgrad_maxwg"))
        while ks > 1 and self.tiles * ks > cap:
            ks -= 1
        return ks

    def ksplit_pairs(self, K, nterm, site):
        """slices of a forward product whose contraction is nterm x K long (operand pairs): the split policy's slice count per term
        times `pairs_ks` ('terms': every term is cut like the plain product -- nterm x as many workgroups; 'same': the plain product's
        workgroup count, each slice nterm x as deep)."""
        ks = self.ksplit_for(K, site=site)
        if nterm == 1 or ks == 1:
            return ks
        return ks * nterm if str(_ab.get("pairs_ks")) == "terms" else ks

    def _names(self, l):
        p = "%s.encoder.layer.%d" % (self.prefix, l)
        a = p + ".attention.self."
        return dict(qkv_w=[a + "query.weight", a + "key.weight", a + "value.weight"],
                    qkv_b=[a + "query.bias", a + "key.bias", a + "value.bias"],
                    o_w=p + ".attention.output.dense.weight", o_b=p + ".attention.output.dense.bias",
                    ln1_g=p + ".attention.output.LayerNorm.weight", ln1_b=p + ".attention.output.LayerNorm.bias",
                    w1=p + ".intermediate.dense.weight", b1=p + ".intermediate.dense.bias",
                    w2=p + ".output.dense.weight", b2=p + ".output.dense.bias",
                    ln2_g=p + ".output.LayerNorm.weight", ln2_b=p + ".output.LayerNorm.bias")

    def param_names(self):
        out = []
        for l in range(self.L):
            nm = self._names(l)
            out += nm["qkv_w"] + nm["qkv_b"] + [nm[k] for k in ("o_w", "o_b", "ln1_g", "ln1_b", "w1", "b1", "w2", "b2", "ln2_g", "ln2_b")]
        return out

    def output(self):
        ws = self.layers[-1]
        return ws["o32"], ws["o16"]

    def output_lo(self):
        """lo half of the bf16 output pair (None without pair_x)."""
        return self.layers[-1]["o16_lo"]

    # ------------------------------------------------------------------------------------------ forward
    def build_forward(self, plan, x32, x16, training, zero_arena=True, x16_lo=None):
        """zero_arena=False: the caller clears self.yarena (split-K accumulation targets) together with its other buffers.
        x16_lo: lo half of the input pair (pair_x; None: the first layer's QKV product reads a plain bf16 input)."""
        fl, dt, T, H, I, S, B = self.flat, self.flat.dt, self.T, self.H, self.I, self.S, self.B
        sm = self.sm
        p = self.p if training else 0.0
        if self.probe_skip:
            return
        if zero_arena:
            plan.add_zeros(([self.yarena] if self.zero_y else []) + ([self.ln_ctr] if self.ln_ctr is not None else []), sm)
        for l, ws in enumerate(self.layers):
            nm = self._names(l)
            plan.wait_point(("layer", self.prefix, l), sm)
            slot = [0]
            wqkv, bqkv = fl.wop_fused(nm["qkv_w"]), fl.w32_fused(nm["qkv_b"])
            qkv = ws["qkv"]
            px, pw = self.pair_x, self.pair_w
            wl = (lambda n: fl.wlo(n)) if pw else (lambda n: None)
            nterm = 1 + int(px) + int(pw)           # terms of a paired product: its split divides nterm x K (UnivlGemm.ksplit)
            qkv_desc = _gemm_desc(dt, x16, H, wqkv, H, T, 3 * H, H, out16=qkv, ldc=3 * H, bias=bqkv,
                                  a_lo=x16_lo if px else None, b_lo=fl.wlo_fused(nm["qkv_w"]) if pw else None)
            o_desc = _gemm_desc(dt, ws["ctx"], H, fl.wop(nm["o_w"]), H, T, H, H, out32=ws["y1"], ldc=H,
                                bias=fl.w32(nm["o_b"]), ksplit=self.ksplit_pairs(H, nterm, "o_fwd"), a_lo=ws["ctx_lo"], b_lo=wl(nm["o_w"]))
            f1_desc = _gemm_desc(dt, ws["a16"], H, fl.wop(nm["w1"]), H, T, I, H, out16=ws["f"], ldc=I,
                                 bias=fl.w32(nm["b1"]), aux=ws["u"], ldaux=I, gelu="fwd", aux_f32=self.u_f32,
                                 a_lo=ws["a16_lo"], b_lo=wl(nm["w1"]), out16_lo=ws["f_lo"])
            f2_desc = _gemm_desc(dt, ws["f"], I, fl.wop(nm["w2"]), I, T, H, I, out32=ws["y2"], ldc=H,
                                 bias=fl.w32(nm["b2"]), ksplit=self.ksplit_pairs(I, nterm, "ffn2_fwd"), a_lo=ws["f_lo"], b_lo=wl(nm["w2"]))
            attn_f = ops.attention_desc(
                dt, B, self.NH, S, S, (qkv, 0), 3 * H, (qkv, H), 3 * H, (qkv, 2 * H), 3 * H, ws["ctx"], H, ws["lse"],
                key_mask=self.key_mask, p_drop=p, offset=ws["off"][0], seed_dev=self.seed_dev, out_lo=ws["ctx_lo"])
            # Which of the four products carry the chunks of layer l + 1.  Below 1536 tokens all four (the 64 x 64 rider kernel, the
            # fused attention forward, the LayerNorm folds -- rounds 3 - 5).  From 1536 tokens on the library answers per product
            # (univl_gemm_rider_fits: the 64 x 128 tile carries, the 128 x 128 / 256 x 256 tiles do not) and the layer's chunks are
            # spread over those that do: a product that does not carry is followed by its share as a launch of its own -- at 128 pairs
            # that was ALL of them, 57 update launches and 0.7 - 1.1 ms of serial HBM time in a step whose products leave HBM idle
            # (profiles/r05_final_bench_b128_kernel_stats.csv).
            carriers, nslots = None, 4
            fused_fwd = (self.bf and T <= int(_ab.get("attn_fuse_fwd_max_rows")) and bool(_ab.get("attn_fuse_fwd")) and
                         S <= int(_ab.get("attn_fuse_fwd_max_seq")) and
                         _AttnFwdFused.accepts(attn_f, qkv_desc))
            # what the products of layer l carry: the chunks of the stack's next layer; behind its LAST layer those of `tail_key` (steps.
            # build_step: the first layer of the stack that runs after this one -- cross encoder / decoder -- instead of a launch in front
            # of the whole forward)
            nkey = (("layer", self.prefix, l + 1) if l + 1 < self.L else self.tail_key) if self.adam_ride else None
            if nkey is not None and T >= 1536:
                fits = [_Rider.fits(d) for d in (qkv_desc, o_desc, f1_desc, f2_desc)]
                fits[0] = fits[0] or fused_fwd           # the fused attention forward carries chunks whatever tile the projection would take
                if not any(fits):
                    fits[2] = True               # nothing carries: the FFN1 product is followed by the whole range
                carriers = {id(d) for d, f in zip((qkv_desc, o_desc, f1_desc, f2_desc), fits) if f}
                nslots = len(carriers)

            def gemm(desc, _l=l, _slot=slot, _car=carriers, _ns=nslots, _key=nkey):
                """a forward product of layer l; with self.adam_ride it can carry a quarter of layer l + 1's optimizer chunks.
                (Equal quarters: with the LayerNorm folds two of the four carrying launches end in a latency-bound tail, but giving them
                a larger share -- or a smaller one -- changes nothing: 2.26 - 2.29 vs 2.23 / 2.27 ms, profiles/r04u_ab_rider_shares.txt.)
                (Round 4, measured and removed: riders ONE LAUNCH ahead instead of one layer ahead -- product k of layer l carrying
                quarter k + 1 of its own layer, so that only the first quarter of a stack's first layer is left to the launches in
                front of the forward: bit-identical, 2.405 / 2.436 / 2.406 vs 2.422 / 2.374 / 2.408 ms per step at 4 pairs,
                profiles/r04h_ab_ride_ahead.txt -- the bytes cost the same wherever they ride.)"""
                if _key is not None and (_car is None or id(desc) in _car):
                    plan.add_gemm_rider(desc, _key, _slot[0], _ns, sm)
                    _slot[0] += 1
                else:
                    plan.add("univl_gemm", desc, sm)

            # Round 5: the q | k | v projection computed INSIDE the attention forward (sequences of at most 64 positions, up to 1536
            # tokens): one launch less on the forward chain; the launch carries the optimizer chunks the projection's launch carried
            if fused_fwd:
                key = nkey
                plan.add_attn_fwd_fused(attn_f, qkv_desc, key, slot[0], nslots, sm)
                slot[0] += 1 if key is not None else 0
            else:
                gemm(qkv_desc)
                plan.add("univl_attention_fwd", attn_f, sm)
            ln_fwd = (lambda d: None) if self.probe_no_ln in ("fwd", "both") else (lambda d: plan.add("univl_layernorm_fwd", d, sm))

            def gemm_ln(desc, lnd, site, _l=l, _slot=slot, _key=nkey):
                """a forward product and the LayerNorm behind it: one launch where the library carries the pair (ln_fold), else two"""
                ctr = self.ln_ctr[_l, site] if self.ln_fold else None
                if ctr is not None and not self.probe_no_ln and _GemmLn.accepts(desc, lnd, ctr):
                    key = _key
                    plan.add_gemm_ln(desc, lnd, ctr, key, _slot[0], 4, sm)
                    _slot[0] += 1 if key is not None else 0
                else:
                    gemm(desc)
                    ln_fwd(lnd)

            gemm_ln(o_desc,
                    ops.layernorm_desc(
                        dt, T, H, x=ws["y1"], residual=x32, gamma=fl.w32(nm["ln1_g"]), beta=fl.w32(nm["ln1_b"]), y=ws["y1"],
                        stats=ws["st1"], out32=ws["a32"], out16=ws["a16"] if self.bf else None, p_pre=p, off_pre=ws["off"][1],
                        seed_dev=self.seed_dev, out16_lo=ws["a16_lo"]), 0)
            gemm(f1_desc)
            gemm_ln(f2_desc,
                    ops.layernorm_desc(
                        dt, T, H, x=ws["y2"], residual=ws["a32"], gamma=fl.w32(nm["ln2_g"]), beta=fl.w32(nm["ln2_b"]), y=ws["y2"],
                        stats=ws["st2"], out32=ws["o32"], out16=ws["o16"] if self.bf else None, p_pre=p, off_pre=ws["off"][2],
                        seed_dev=self.seed_dev, out16_lo=ws["o16_lo"]), 1)
            x32, x16, x16_lo = ws["o32"], ws["o16"], ws["o16_lo"]

    # ----------------------------------------------------------------------------------------- backward
    def build_backward(self, plan, gin, x0_32, x0_16, gs, training, layer_hook=None):
        """Emit the whole backward; returns the buffer holding the gradient wrt the stack input."""
        for _ in self.backward_layers(plan, gin, x0_32, x0_16, gs, training, layer_hook):
            pass
        return self.bwd_out

    def backward_layers(self, plan, gin, x0_32, x0_16, gs, training, layer_hook=None, zero_arena=True):
        """Generator form: emits one layer per next() (last layer first) so that a caller can interleave two stacks in
        plan order; self.bwd_out holds the gradient wrt the stack input once exhausted.
        gin: fp32 [T,H] gradient wrt the last layer's output.  `gs` (GradState) decides beta = 0 / 1 per
        weight-gradient GEMM.

        The chain LayerNorm backward -> dgrad -> ... -> dgrad runs on stream `sm`; the four weight-gradient GEMMs of a
        layer only CONSUME that chain's tensors and are issued as one grouped launch at the end of the layer."""
        fl, dt, T, H, I, S, B = self.flat, self.flat.dt, self.T, self.H, self.I, self.S, self.B
        sm = self.sm
        p = self.p if training else 0.0
        self.bwd_out = gin
        if self.probe_skip:
            return
        if zero_arena:
            plan.add_zeros(([self.garena] if self.zero_g else []) + ([self.ln_ctr_b] if self.ln_ctr_b is not None else []), sm)
        # Weight gradients over thousands of tokens (UNIVL_WGRAD_BIG_MIN, bf16): the layer's grouped launch on the 128 x 128 tile
        # (two stages, 4 waves) with the two bias gradients it used to carry on a column-sum kernel instead.  The column-0
        # workgroups of a product with a fused bias gradient walk their staged A tile element by element every K step; with
        # a deep contraction they are the stragglers the whole launch waits for -- isolated at 6144 tokens a layer's group runs
        # 231 us (64 tile, fused bias gradients, the former plan), 185 us (64 tile without them), 138 us (128 tile, 2 stages,
        # 4 waves, without them): profiles/r03w_gemm_group_variants_b128.txt, r03y2_gemm_group_variants_nodbias_b128.txt.
        # From where on: by default exactly where the weight gradients stop riding with their dgrad products anyway -- every dgrad of
        # the layer on the 128 tile (>= 256 tiles for the narrowest output, H columns: 5462 tokens at H = 768; gemm.hip choose /
        # univl_gemm_pair) -- which is the regime the measurements cover (6144 and 12288 tokens); UNIVL_WGRAD_BIG_MIN = tokens overrides.
        big_min = _ab.get("wgrad_big_min")
        big_wgrad = self.bf and (T >= big_min if big_min else ((T + 127) // 128) * ((H + 127) // 128) >= 256)
        # Round 5: from 1536 tokens on (multiples of 256) the grouped launch runs on the 256 x 256 8-phase body (csrc/gemm256.h; the C side
        # picks it for tile = 0 -- `auto256`: 121 vs 147 us per layer at 6144 tokens, profiles/r05c_mb_gemm256.txt); g256=0 keeps the 128 tile.
        wg_tile = {} if self.g256 else (dict(tile=128, stages=2, waves=4) if big_wgrad else {})
        pair_square = _ab.get("pair_form") == "square"
        ln2_folded = False
        for l in range(self.L - 1, -1, -1):
            ws, nm = self.layers[l], self._names(l)
            xin32, xin16 = (x0_32, x0_16) if l == 0 else (self.layers[l - 1]["o32"], self.layers[l - 1]["o16"])
            sc = self.scr
            s_dxd, s_dxd2, s_du, s_dqkv = sc["dxd"], sc["dxd2"], sc["du"], sc["dqkv"]
            dz, da = self.gbuf, self.garena[l, 0]
            ln_bwd = (lambda d: None) if self.probe_no_ln in ("bwd", "both") else (lambda d: plan.add("univl_layernorm_bwd", d, sm))

            def ln2_desc(_l, _gin):
                """output LayerNorm / dropout backward of layer _l (BertOutput, module_bert.py:246-250)"""
                _ws, _nm = self.layers[_l], self._names(_l)
                return ops.layernorm_desc(
                    dt, T, H, gamma=fl.w32(_nm["ln2_g"]), y=_ws["y2"], stats=_ws["st2"], dout=_gin, dx32=self.gbuf, dxd16=s_dxd,
                    dgamma=fl.g(_nm["ln2_g"]), dbeta=fl.g(_nm["ln2_b"]), dbias=fl.g(_nm["b2"]), p_pre=p, off_pre=_ws["off"][2],
                    seed_dev=self.seed_dev)

            if not ln2_folded:               # (folded: the QKV pair launch of the layer above finished it, see the end of the loop body)
                ln_bwd(ln2_desc(l, gin))
            ln2_folded = False
            wgrads = []                      # the weight gradients that do not ride with their dgrad: the layer's grouped launch

            def emit(dgrad, wgrad, lnd=None, site=0, _l=l):
                """dgrad on the chain; its weight-gradient twin either into the layer's grouped launch (default) or into the
                SAME launch (self.ride, where the C side accepts the pair: bf16, 64 x 64 tiles).  lnd: the LayerNorm backward that
                consumes the dgrad's output -- finished inside the pair launch where the library carries it (returns True), else the
                caller enqueues it."""
                if pair_square:
                    dgrad.tile = 64          # A/B switch UNIVL_PAIR_FORM=square: an explicit tile keeps the 64 x 64 form of the pair launch
                if (lnd is not None and self.ride and self.ln_fold_bwd and not self.probe_no_ln and
                        _PairLn.accepts(dgrad, wgrad, lnd, self.ln_ctr_b[_l, site])):
                    plan.add_gemm_pair_ln(dgrad, wgrad, lnd, self.ln_ctr_b[_l, site], sm)
                    return True
                if self.ride and _Pair.accepts(dgrad, wgrad):
                    plan.add_gemm_pair(dgrad, wgrad, sm)
                else:
                    plan.add("univl_gemm", dgrad, sm)
                    wgrads.append(wgrad)
                return False

            w_ffn2 = _gemm_desc(dt, s_dxd, H, ws["f"], I, H, I, T, trans_a=1, trans_b=1,
                                out32=fl.g(nm["w2"]), ldc=I, accumulate=gs.acc(nm["w2"]), **wg_tile, **gs.sumsq_args(nm["w2"], H, I))
            emit(_gemm_desc(dt, s_dxd, H, fl.wop(nm["w2"]), I, T, I, H, trans_b=1, out16=s_du,
                            ldc=I, aux=ws["u"], ldaux=I, gelu="bwd", aux_f32=self.u_f32), w_ffn2)
            # Bias gradients of the two projections whose upstream gradient no LayerNorm kernel sees (FFN1, QKV): the descriptors carry
            # `dbias`; the pair launch and the big-tile grouped launch take them as column-sum workgroups of their own (gemm.hip
            # colsum_tile, round 4), the 64-tile grouped launch from the operand tiles it stages anyway.
            w_ffn1 = _gemm_desc(dt, s_du, I, ws["a16"], H, I, H, T, trans_a=1, trans_b=1,
                                out32=fl.g(nm["w1"]), ldc=H, accumulate=gs.acc(nm["w1"]), dbias=fl.g(nm["b1"]),
                                **wg_tile, **gs.sumsq_args(nm["w1"], I, H))
            # attention-output LayerNorm / dropout backward (BertSelfOutput, module_bert.py:207-211), fed by the FFN1 dgrad
            dy = self.gbuf
            ln1 = ops.layernorm_desc(
                dt, T, H, gamma=fl.w32(nm["ln1_g"]), y=ws["y1"], stats=ws["st1"], dout=da, dx32=dy, dxd16=s_dxd2,
                dgamma=fl.g(nm["ln1_g"]), dbeta=fl.g(nm["ln1_b"]), dbias=fl.g(nm["o_b"]), p_pre=p, off_pre=ws["off"][1],
                seed_dev=self.seed_dev)
            if not emit(_gemm_desc(dt, s_du, I, fl.wop(nm["w1"]), H, T, H, I, trans_b=1, out32=da, ldc=H,
                                   residual=dz, ldr=H, ksplit=self.ksplit_for(I, dgrad=True, site="ffn1_dgrad")), w_ffn1, ln1, 0):
                ln_bwd(ln1)
            w_o = _gemm_desc(dt, s_dxd2, H, ws["ctx"], H, H, H, T, trans_a=1, trans_b=1,
                             out32=fl.g(nm["o_w"]), ldc=H, accumulate=gs.acc(nm["o_w"]), **wg_tile, **gs.sumsq_args(nm["o_w"], H, H))
            o_dgrad = _gemm_desc(dt, s_dxd2, H, fl.wop(nm["o_w"]), H, T, H, H, trans_b=1, out16=self.dctx, ldc=H)
            qkv, dqkv = ws["qkv"], s_dqkv
            attn_b = ops.attention_desc(
                dt, B, self.NH, S, S, (qkv, 0), 3 * H, (qkv, H), 3 * H, (qkv, 2 * H), 3 * H, ws["ctx"], H, ws["lse"],
                key_mask=self.key_mask, p_drop=p, offset=ws["off"][0], seed_dev=self.seed_dev, dout=self.dctx, lddo=H,
                dq=(dqkv, 0), lddq=3 * H, dk=(dqkv, H), lddk=3 * H, dv=(dqkv, 2 * H), lddv=3 * H)
            # Round 5: the attention-output dgrad computed INSIDE the attention backward (one launch and one [tokens, 768] round trip
            # less on the chain; sequences of at most 64 positions), its weight gradient riding there where weight gradients ride
            # (below 1536 tokens: at 6144 every one of the 3072 role workgroups walks a K loop of its own in front of the attention body --
            #  11.87 vs 11.32 ms per step at 128 pairs; 2.26 vs 2.31 at 4 pairs, 3.37 vs 3.43 at 16: profiles/r05p_ab_attn_fuse_bwd.txt)
            w_ride = w_o if self.ride else None
            if (self.bf and T <= int(_ab.get("attn_fuse_bwd_max_rows")) and bool(_ab.get("attn_fuse_bwd")) and
                    _AttnBwdFused.accepts(attn_b, o_dgrad, w_ride)):
                plan.add_attn_bwd_fused(attn_b, o_dgrad, w_ride, sm)
                if w_ride is None:
                    wgrads.append(w_o)
            else:
                emit(o_dgrad, w_o)
                plan.add("univl_attention_bwd", attn_b, sm)
            w_qkv = _gemm_desc(dt, dqkv, 3 * H, xin16, H, 3 * H, H, T, trans_a=1, trans_b=1,
                               out32=fl.g_fused(nm["qkv_w"]), ldc=H, accumulate=gs.acc(nm["qkv_w"][0]),
                               dbias=fl.g_fused(nm["qkv_b"]), **wg_tile,
                               **gs.sumsq_args(nm["qkv_w"], H, H))
            dx = self.garena[l, 1]
            # ... the QKV dgrad feeds the output LayerNorm backward of the layer BELOW (next iteration)
            ln2_folded = emit(_gemm_desc(dt, dqkv, 3 * H, fl.wop_fused(nm["qkv_w"]), H, T, H, 3 * H, trans_b=1,
                                         out32=dx, ldc=H, residual=dy, ldr=H, ksplit=self.ksplit_for(3 * H, dgrad=True, site="qkv_dgrad")), w_qkv,
                                      ln2_desc(l - 1, dx) if (l > 0 and not wgrads) else None, 1)   # (a deferred weight gradient of this layer still reads s_dxd, which the folded LayerNorm overwrites)
            # the layer's four weight-gradient GEMMs only consume tensors the chain above produced (dxd, du, dxd2, dqkv
            # are distinct buffers): one grouped launch, after which the scratch may be reused by the next layer
            if wgrads:                                  # (self.ride: empty -- every weight gradient went out with its dgrad)
                plan.add_gemm_group(wgrads, sm)
            gin = dx
            if layer_hook is not None:
                layer_hook(plan, self.prefix, l, sm)
            self.bwd_out = gin
            yield l
        self.bwd_out = gin


class DecoderLayer:
    """What training (DecoderStack.build_forward) and cached decoding (decode.CachedDecoder._step_plan) share of a decoder layer
    (module_decoder.py:268-320), stated once: emitters over one layer's workspace of T rows (DecoderStack.layer_workspace).  The
    self-attention core stays with each caller.  p / off / seed_dev: dropout probability, the layer's five stream offsets, the seed word."""

    H, NH, I = 768, 12, 3072
    BLOCK = {"s_": ("1", "a", 1), "c_": ("2", "d", 3)}     # name prefix -> workspace suffix, output buffer, dropout offset

    def __init__(self, plan, flat, l, ws, T, p=0.0, off=(0, 0, 0, 0, 0), seed_dev=None, stream=0):
        self.plan, self.fl, self.nm, self.ws, self.T = plan, flat, DecoderStack._names(l), ws, T
        self.p, self.off, self.seed_dev, self.sm = p, off, seed_dev, stream

    def _gemm(self, desc):
        self.plan.add("univl_gemm", desc, self.sm)

    def _res_ln(self, sfx, residual, g, b, out, off):
        fl, ws, nm = self.fl, self.ws, self.nm
        self.plan.add("univl_layernorm_fwd", ops.layernorm_desc(
            fl.dt, self.T, self.H, x=ws["y" + sfx], residual=residual, gamma=fl.w32(nm[g]), beta=fl.w32(nm[b]), y=ws["y" + sfx],
            stats=ws["st" + sfx], out32=ws[out + "32"], out16=ws[out + "16"] if fl.compute_dtype == torch.bfloat16 else None,
            p_pre=self.p, off_pre=off, seed_dev=self.seed_dev), self.sm)

    def attn_output(self, pre, x32):
        """output dense + residual LayerNorm of the self-attention ("s_") or encoder-attention ("c_") block; x32: the block's input"""
        fl, ws, nm, H = self.fl, self.ws, self.nm, self.H
        sfx, out, oi = self.BLOCK[pre]
        self._gemm(_gemm_desc(fl.dt, ws["ctx" + sfx], H, fl.wop(nm[pre + "o_w"]), H, self.T, H, H, out32=ws["y" + sfx], ldc=H,
                              bias=fl.w32(nm[pre + "o_b"])))
        self._res_ln(sfx, x32, pre + "ln_g", pre + "ln_b", out, self.off[oi])

    def enc_query(self):
        fl, ws, nm, H = self.fl, self.ws, self.nm, self.H
        self._gemm(_gemm_desc(fl.dt, ws["a16"], H, fl.wop_fused(nm["c_q_w"]), H, self.T, H, H, out16=ws["q2"], ldc=H,
                              bias=fl.w32_fused(nm["c_q_b"])))

    def enc_attention(self, B, Sq, Sk, kv, key_mask):
        """B x Sq query rows (= T) over the Sk encoder positions of their instance; kv: [B * Sk, 2H] keys | values"""
        ws, H = self.ws, self.H
        self.plan.add("univl_attention_fwd", ops.attention_desc(
            self.fl.dt, B, self.NH, Sq, Sk, ws["q2"], H, (kv, 0), 2 * H, (kv, H), 2 * H, ws["ctx2"], H, ws["lse2"],
            key_mask=key_mask, p_drop=self.p, offset=self.off[2], seed_dev=self.seed_dev), self.sm)

    def ffn(self, big=None):
        """FFN1 + GELU, FFN2, residual LayerNorm; big: how the caller adds the two products (None: plainly)"""
        fl, ws, nm, H, I = self.fl, self.ws, self.nm, self.H, self.I
        add = big or self._gemm
        add(_gemm_desc(fl.dt, ws["d16"], H, fl.wop(nm["w1"]), H, self.T, I, H, out16=ws["f"], ldc=I, bias=fl.w32(nm["b1"]),
                       aux=ws["u"], ldaux=I, gelu="fwd"))
        add(_gemm_desc(fl.dt, ws["f"], I, fl.wop(nm["w2"]), I, self.T, H, I, out32=ws["y3"], ldc=H, bias=fl.w32(nm["b2"])))
        self._res_ln("3", ws["d32"], "ln_g", "ln_b", "o", self.off[4])


class DecoderStack:
    """Decoder of module_decoder.py:322-340: L layers of {causal self-attention, encoder attention over the cross
    encoder output, FFN}, each followed by the BertSelfOutput / BertOutput residual + LayerNorm blocks
    (module_decoder.py:268-292).  Tq = B*Wd decoder tokens, Tkv = B*Sk encoder tokens."""

    H, NH, I = 768, 12, 3072

    def __init__(self, flat, n_layers, B, Wd, Sk, dec_mask, enc_mask, p_drop, seed_dev, sites, stream=0):
        self.flat, self.L, self.B, self.Wd, self.Sk = flat, n_layers, B, Wd, Sk
        self.Tq, self.Tkv = B * Wd, B * Sk
        self.dec_mask, self.enc_mask = dec_mask, enc_mask
        self.p, self.seed_dev, self.sm = float(p_drop), seed_dev, stream
        dev, H, I, Tq, Tkv = flat.device, self.H, self.I, self.Tq, self.Tkv
        ct = flat.compute_dtype
        e = _workspace(dev)
        self.layers = []
        for l in range(n_layers):
            ws = self.layer_workspace(e, ct, Tq)
            ws.update(qkv=e(Tq, 3 * H, dtype=ct), kv2=e(Tkv, 2 * H, dtype=ct), off=[sites.next() for _ in range(5)])
            self.layers.append(ws)
        self.g1, self.g2 = e(Tq, H), e(Tq, H)
        self.dxd = e(Tq, H, dtype=ct)
        self.du = e(Tq, I, dtype=ct)
        self.dctx = e(Tq, H, dtype=ct)
        self.dqkv = e(Tq, 3 * H, dtype=ct)
        self.dq2 = e(Tq, H, dtype=ct)
        self.dkv2 = e(Tkv, 2 * H, dtype=ct)

    @classmethod
    def layer_workspace(cls, e, ct, T):
        """One layer's buffers for T decoder rows from the caller's allocator e (this class adds qkv, kv2, off; decoding adds q1)."""
        H, I = cls.H, cls.I
        ws = dict(ctx1=e(T, H, dtype=ct), lse1=e(T * cls.NH), y1=e(T, H), st1=e(T, 2), a32=e(T, H),
                  q2=e(T, H, dtype=ct), ctx2=e(T, H, dtype=ct), lse2=e(T * cls.NH), y2=e(T, H), st2=e(T, 2), d32=e(T, H),
                  u=e(T, I, dtype=ct), f=e(T, I, dtype=ct), y3=e(T, H), st3=e(T, 2), o32=e(T, H))
        for k in ("a", "d", "o"):
            ws[k + "16"] = e(T, H, dtype=ct) if ct == torch.bfloat16 else ws[k + "32"]
        return ws

    @staticmethod
    def _names(l):
        p = "decoder.decoder.layer.%d" % l
        s, c = p + ".slf_attn", p + ".enc_attn"
        qkv = lambda a, names, suf: [a + ".att." + n + suf for n in names]
        return dict(s_qkv_w=qkv(s, ("query", "key", "value"), ".weight"), s_qkv_b=qkv(s, ("query", "key", "value"), ".bias"),
                    s_o_w=s + ".output.dense.weight", s_o_b=s + ".output.dense.bias",
                    s_ln_g=s + ".output.LayerNorm.weight", s_ln_b=s + ".output.LayerNorm.bias",
                    c_q_w=qkv(c, ("query",), ".weight"), c_q_b=qkv(c, ("query",), ".bias"),
                    c_kv_w=qkv(c, ("key", "value"), ".weight"), c_kv_b=qkv(c, ("key", "value"), ".bias"),
                    c_o_w=c + ".output.dense.weight", c_o_b=c + ".output.dense.bias",
                    c_ln_g=c + ".output.LayerNorm.weight", c_ln_b=c + ".output.LayerNorm.bias",
                    w1=p + ".intermediate.dense.weight", b1=p + ".intermediate.dense.bias",
                    w2=p + ".output.dense.weight", b2=p + ".output.dense.bias",
                    ln_g=p + ".output.LayerNorm.weight", ln_b=p + ".output.LayerNorm.bias")

    def output(self):
        return self.layers[-1]["o32"], self.layers[-1]["o16"]

    def build_forward(self, plan, x32, x16, enc16, training):
        fl, dt, H, B, Wd, Sk, Tq, Tkv, sm = self.flat, self.flat.dt, self.H, self.B, self.Wd, self.Sk, self.Tq, self.Tkv, self.sm
        p = self.p if training else 0.0
        adam_ride = (getattr(fl, "adam_ride", False)
                     and fl.compute_dtype == torch.bfloat16 and training)
        for l, ws in enumerate(self.layers):
            plan.wait_point(("layer", "decoder", l), sm)
            slot = [0]

            def big(desc, _l=l, _slot=slot):
                """one of the layer's four large forward products: with the riding optimizer update it carries a quarter of the
                chunks of layer l + 1 (Plan.add_gemm_rider; the decoder runs once per forward, on one stream)"""
                if adam_ride and _l + 1 < self.L:
                    plan.add_gemm_rider(desc, ("layer", "decoder", _l + 1), _slot[0], 4, sm)
                    _slot[0] += 1
                else:
                    plan.add("univl_gemm", desc, sm)

            lay = DecoderLayer(plan, fl, l, ws, Tq, p, ws["off"], self.seed_dev, sm)
            nm, qkv, kv = lay.nm, ws["qkv"], ws["kv2"]
            big(_gemm_desc(dt, x16, H, fl.wop_fused(nm["s_qkv_w"]), H, Tq, 3 * H, H, out16=qkv, ldc=3 * H,
                           bias=fl.w32_fused(nm["s_qkv_b"])))
            plan.add("univl_attention_fwd", ops.attention_desc(
                dt, B, self.NH, Wd, Wd, (qkv, 0), 3 * H, (qkv, H), 3 * H, (qkv, 2 * H), 3 * H, ws["ctx1"], H, ws["lse1"],
                key_mask=self.dec_mask, causal=True, p_drop=p, offset=ws["off"][0], seed_dev=self.seed_dev), sm)
            lay.attn_output("s_", x32)
            lay.enc_query()
            big(_gemm_desc(dt, enc16, H, fl.wop_fused(nm["c_kv_w"]), H, Tkv, 2 * H, H, out16=kv, ldc=2 * H, bias=fl.w32_fused(nm["c_kv_b"])))
            lay.enc_attention(B, Wd, Sk, kv, self.enc_mask)
            lay.attn_output("c_", ws["a32"])
            lay.ffn(big)
            x32, x16 = ws["o32"], ws["o16"]

    def build_backward(self, plan, gin, x0_32, x0_16, enc16, denc32, gs, training):
        """gin: grad wrt the last layer output [Tq,H] fp32.  denc32 [Tkv,H] fp32 is ACCUMULATED into (every layer's
        encoder-attention K/V projections read the same cross-encoder output).  Returns the grad wrt the stack input.

        Every weight-gradient product goes out in the launch of the dgrad product fed by the same upstream gradient
        (Plan.add_gemm_pair, as in EncoderStack: the weight-gradient tiles fill the compute units the latency-bound dgrad leaves
        idle) where the C side takes the pair (bf16, 64 x 64 tiles); otherwise the two launches one after the other."""
        fl, dt, H, I, B, Wd, Sk, Tq, Tkv, sm = self.flat, self.flat.dt, self.H, self.I, self.B, self.Wd, self.Sk, self.Tq, self.Tkv, self.sm
        p = self.p if training else 0.0
        G = fl.g
        ride = (bool(_ab.get("wgrad_ride")) and bool(_ab.get("decoder_pair"))
                and fl.compute_dtype == torch.bfloat16)

        def emit(wgrad, dgrad):
            if ride and _Pair.accepts(dgrad, wgrad):
                plan.add_gemm_pair(dgrad, wgrad, sm)
            else:
                plan.add("univl_gemm", wgrad, sm)
                plan.add("univl_gemm", dgrad, sm)

        def proj_pair(dy, x16, wn, bn, rows, out32, **kw):
            """wgrad + dgrad pair of y = x16 . W^T + b given dy [rows, N]; wn / bn: weight / bias names; kw: how the dgrad lands in out32"""
            N = dy.shape[1]
            emit(_gemm_desc(dt, dy, N, x16, H, N, H, rows, trans_a=1, trans_b=1, out32=fl.g_fused(wn), ldc=H,
                            accumulate=gs.acc(wn[0]), dbias=fl.g_fused(bn)),
                 _gemm_desc(dt, dy, N, fl.wop_fused(wn), H, rows, H, N, trans_b=1, out32=out32, ldc=H, **kw))

        for l in range(self.L - 1, -1, -1):
            ws, nm = self.layers[l], self._names(l)
            off = ws["off"]
            xin16 = x0_16 if l == 0 else self.layers[l - 1]["o16"]

            def attn_block(pre, dout, attn, dq, x16, kv=None):
                """The self- ("s_") / encoder-attention ("c_") block's backward given dout: LayerNorm, output projection, attention
                (attn: its descriptor), then the input projections -- the encoder K/V one (kv = (dkv, enc16), accumulated into denc32)
                and dq against the block input x16 plus the LayerNorm's dx (residual path).  Returns the gradient wrt x16's block input."""
                sfx, _, oi = DecoderLayer.BLOCK[pre]
                plan.add("univl_layernorm_bwd", ops.layernorm_desc(
                    dt, Tq, H, gamma=fl.w32(nm[pre + "ln_g"]), y=ws["y" + sfx], stats=ws["st" + sfx], dout=dout, dx32=self.g1,
                    dxd16=self.dxd, dgamma=G(nm[pre + "ln_g"]), dbeta=G(nm[pre + "ln_b"]), dbias=G(nm[pre + "o_b"]), p_pre=p,
                    off_pre=off[oi], seed_dev=self.seed_dev), sm)
                emit(_gemm_desc(dt, self.dxd, H, ws["ctx" + sfx], H, H, H, Tq, trans_a=1, trans_b=1, out32=G(nm[pre + "o_w"]),
                                ldc=H, accumulate=gs.acc(nm[pre + "o_w"])),
                     _gemm_desc(dt, self.dxd, H, fl.wop(nm[pre + "o_w"]), H, Tq, H, H, trans_b=1, out16=self.dctx, ldc=H))
                plan.add("univl_attention_bwd", attn, sm)
                if kv is not None:
                    proj_pair(kv[0], kv[1], nm["c_kv_w"], nm["c_kv_b"], Tkv, denc32, accumulate=True)
                qn = "c_q" if kv is not None else "s_qkv"
                proj_pair(dq, x16, nm[qn + "_w"], nm[qn + "_b"], Tq, self.g2, residual=self.g1, ldr=H)
                return self.g2

            # FFN block
            dz = self.g1
            plan.add("univl_layernorm_bwd", ops.layernorm_desc(
                dt, Tq, H, gamma=fl.w32(nm["ln_g"]), y=ws["y3"], stats=ws["st3"], dout=gin, dx32=dz, dxd16=self.dxd,
                dgamma=G(nm["ln_g"]), dbeta=G(nm["ln_b"]), dbias=G(nm["b2"]), p_pre=p, off_pre=off[4], seed_dev=self.seed_dev), sm)
            emit(_gemm_desc(dt, self.dxd, H, ws["f"], I, H, I, Tq, trans_a=1, trans_b=1, out32=G(nm["w2"]), ldc=I,
                            accumulate=gs.acc(nm["w2"])),
                 _gemm_desc(dt, self.dxd, H, fl.wop(nm["w2"]), I, Tq, I, H, trans_b=1, out16=self.du, ldc=I,
                            aux=ws["u"], ldaux=I, gelu="bwd"))
            dd = self.g2
            proj_pair(self.du, ws["d16"], [nm["w1"]], [nm["b1"]], Tq, dd, residual=dz, ldr=H)
            kv, dkv, qkv, dqkv = ws["kv2"], self.dkv2, ws["qkv"], self.dqkv
            da = attn_block("c_", dd, ops.attention_desc(
                dt, B, self.NH, Wd, Sk, ws["q2"], H, (kv, 0), 2 * H, (kv, H), 2 * H, ws["ctx2"], H, ws["lse2"],
                key_mask=self.enc_mask, p_drop=p, offset=off[2], seed_dev=self.seed_dev, dout=self.dctx, lddo=H,
                dq=self.dq2, lddq=H, dk=(dkv, 0), lddk=2 * H, dv=(dkv, H), lddv=2 * H), self.dq2, ws["a16"], kv=(dkv, enc16))
            gin = attn_block("s_", da, ops.attention_desc(
                dt, B, self.NH, Wd, Wd, (qkv, 0), 3 * H, (qkv, H), 3 * H, (qkv, 2 * H), 3 * H, ws["ctx1"], H, ws["lse1"],
                key_mask=self.dec_mask, causal=True, p_drop=p, offset=off[0], seed_dev=self.seed_dev, dout=self.dctx, lddo=H,
                dq=(dqkv, 0), lddq=3 * H, dk=(dqkv, H), lddk=3 * H, dv=(dqkv, 2 * H), lddv=3 * H), dqkv, xin16)
        return gin
