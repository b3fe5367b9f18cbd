"""The async slots (sn_submit / sn_submit_nv12 / sn_wait: DnnNode::Run with is_sync_mode = false) held to the synchronous call.
From the second use of a slot's cell on a request is a captured hipGraph of {H2D, forward, D2H}, looked up in
Slot::gexec[input kind][output mask][arithmetic x (alone | sharing the GPU)] (submit_common): every kernel argument, grid and
memset of forward() is frozen at capture time, and a capture that fails turns the graphs off without a word.  Needs an MI355X.

Which cell a request hits is host state, not GPU timing (submit_common): a request takes the first slot in index order whose
ticket is 0, a ticket is cleared by sn_wait alone, `shared` is 1 exactly when another slot holds an un-waited ticket, and
mi = (F16X3 ? 0 : 2) + shared.  A cell's first use is plain launches, its second is captured and launched from the graph,
later uses are replays.  So:  slot 0 alone = submit, wait, submit, wait ...;  slot 1 sharing = hold one un-waited ticket on
slot 0, then submit and wait;  slot 0 sharing = hold the ticket on slot 1 (submit A, submit B, wait A).  Slot 1 alone cannot
be reached: slot 1 is taken only while slot 0 is owned.  sn_dbg_slot_graphs (api.dbg_slot_graphs) reads what the slots did:
whether the graphs are still on, graphs instantiated, requests served by hipGraphLaunch.  Five uses of a fresh cell must read
+1 / +4 with the graphs still on: those counts are the point, a run in which they are 0 has compared plain launches.

The comparison target is always the synchronous call of the same frame on the same handle in the same forced arithmetic
(eng.infer, eng.infer_sbs_nv12 for a camera frame), bit for bit on raw and disp, never a second async run; on an SN_PREC_AUTO
handle (d) it is the forced handles' maps, as tests/test_gpu_auto_sequences.py.  User buffers are views GUARD words inside
larger arrays; view and guards are poisoned before every submit, the guards must be intact after the wait, and a buffer that
was not asked for must not be written anywhere.  Every submit has a finite timeout (20000 ms): a slot that is not handed back
fails the test with SN_ERR_BUSY instead of hanging it.

Geometries of (a): 96x64 D 48 (the suite's async fixture); 124x38 D 32 (padded right and bottom); the hierarchical model at
96x64 D 48 (refine_coarse inside the graph); and a share-size geometry, `share_geometry`: ws.tower_cu = num_cu * 7 / 8 changes
a streamed launch only if ceil(rows / num_cu) != ceil(rows / tower_cu) (launch_ref_block_stream*: rows_per_wg), rows being the
flat rows of one pair (tower_ref.stream_sched).  At 96x64 both grids give every workgroup one row (128 rows), and at 96x320
both give three (640 rows, 214 workgroups either way): neither sharing cell there is a different schedule.  With 256 CUs the
smallest height at width 64 at which EVERY streamed launch of both towers differs is 226 (padded 240: 480 rows = 2 against 3
per workgroup, 240 rows for the wide strips of dilation 4 / 8 = 1 against 2, the tail form's 452 rows = 2 against 3).  The test
computes it from the device's CU count and checks the two grids on the device through sn_dbg_set_grid_cus / sn_dbg_last_launch.

(c) uses truth_compare's overflowing points S-tower+16 and S-low+16 with F16 forced.  No input is clean under either model:
on the CPU (truth_compare.range_profile) the tower model's stored activations reach 1.6e5 for the all-zero frame and 3.8e5 ..
6.8e5 for max / min / noise / checker / step / seeds 4-6, and the low model's reach 7.1e4 for the all-zero frame (constant
frames of -64 .. 64: 6.8e4 at the least, for -1) against 65504.  So, as the issue allows, the two points alternate on two
handles, each over one cell past its capture: a replay that did not clear ws.stats would hand the next ticket the sum of
the counts (every pixel of every frame is flagged under these models: 15648 per ticket, and 60 low-resolution pixels under
the low model).  The clean side (SN_OK, all counts zero, equal to the synchronous call's) is every ticket of (a).

The `async_graph|` lines are profiles/async_graph_cells.txt."""
import collections
import ctypes as C
import threading
import time

import numpy as np
import pytest

import tower_ref as tr
import truth_compare as tc
from hobot_stereonet_amd import api, synth, weights

pytestmark = pytest.mark.gpu

TIMEOUT_MS = 20000           # every submit: the convention of test_the_sequence_through_submit_and_wait
USES = 5                     # per cell: plain, capture + launch, three replays
GUARD = 64                   # words on either side of a user buffer
POISON = 0x5A5A5A5A
KIND = ("tensor", "nv12")
MASK = {1: "raw", 2: "disp", 3: "both"}
STAT_KEYS = ("level_px", "residual_px", "nonfinite_px", "nonfinite_low_px", "precision_last")
SN_ERR_ARG, SN_ERR_BUSY, SN_ERR_TICKET = -1, -6, -7
REF_DIL = (1, 2, 4, 8, 1, 1)          # kRefDil (sn_engine.hpp)

Ref = collections.namedtuple("Ref", "disp raw stats")


class Out:
    """one user output: an (h, w) view GUARD words inside a larger array"""

    def __init__(self, h, w, dtype):
        self.big = np.empty(2 * GUARD + h * w, dtype)
        self.view = self.big[GUARD:GUARD + h * w].reshape(h, w)
        assert self.view.flags["C_CONTIGUOUS"] and self.view.base is not None
        self.poison()

    def poison(self):
        self.big.view(np.uint32)[:] = POISON

    def guards_intact(self):
        u = self.big.view(np.uint32)
        return bool((u[:GUARD] == POISON).all() and (u[-GUARD:] == POISON).all())

    def untouched(self):
        return bool((self.big.view(np.uint32) == POISON).all())


def _bits_differ(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


class Req:
    """one submit into freshly poisoned buffers; mask: 1 = raw, 2 = disp, 3 = both (the other buffer is passed as None)"""

    def __init__(self, eng, kind, frame, mask, timeout_ms=TIMEOUT_MS):
        self.eng, self.mask = eng, mask
        self.raw, self.disp = Out(eng.height, eng.width, np.int32), Out(eng.height, eng.width, np.float32)
        self.ticket = (eng.submit_nv12 if kind else eng.submit)(frame, self.raw.view if mask & 1 else None,
                                                               self.disp.view if mask & 2 else None, timeout_ms=timeout_ms)
        self.flag = None

    def wait(self):
        """-> infer_ms; an SN_ERR_RANGE is kept in .flag (the maps were copied and the ticket is consumed)"""
        try:
            return self.eng.wait(self.ticket)
        except api.StereoNetRangeError as e:
            self.flag = e
            return float("nan")

    def judge(self, disp, raw):
        """-> (misses, differing elements) against the synchronous maps of the request's frame"""
        bad, differing = [], 0
        for name, out, ref, asked in (("raw", self.raw, raw, self.mask & 1), ("disp", self.disp, disp, self.mask & 2)):
            if asked:
                if not out.guards_intact():
                    bad.append(f"{name}: a guard word was written")
                d = _bits_differ(out.view, ref)
                differing += d
                if d:
                    bad.append(f"{name}: {d} elements differ from the synchronous call's")
            elif not out.untouched():
                bad.append(f"{name} was not asked for and was written")
        return bad, differing


def _sync_ref(eng, kind, frame):
    disp, raw = eng.infer_sbs_nv12(frame) if kind else eng.infer(frame)
    st = eng.refine_stats()
    return Ref(disp, raw, {k: st[k] for k in STAT_KEYS})


def _frames(w, h, d, n=USES, seed0=60):
    """-> (tensor frames, side-by-side NV12 frames): n different frames of each kind"""
    return ([synth.model_input_i8(w, h, d, seed0 + i) for i in range(n)],
            [synth.sbs_nv12_frame(w, h, d, seed0 + 20 + i) for i in range(n)])


def _drive(eng, tag, kind, mask, how, frames, refs, expect=(1, 4, 1), uses=USES, stat_bad=None):
    """`uses` requests, one at a time, into the cell the caller has arranged (how: 'slot0 alone', ...): every ticket's maps
    and statistic against the synchronous call of its frame, then the read-out against `expect` = (instantiated, launches)
    risen by, enabled.  -> misses; those of the statistic go to `stat_bad` instead where the caller judges them apart"""
    _, inst0, la0 = eng.dbg_slot_graphs()
    bad, ms, differing, stat_differs = [], [], 0, 0
    for u in range(uses):
        calls0 = eng.refine_stats()["calls"]
        req = Req(eng, kind, frames[kind][u], mask)
        ms.append(req.wait())
        ref = refs[kind][u]
        msgs, d = req.judge(ref.disp, ref.raw)
        differing += d
        st = eng.refine_stats()
        if req.flag is not None:
            msgs.append(f"flagged: {req.flag}")
        smsgs = [f"{k} {st[k]!r} is not the synchronous call's {ref.stats[k]!r}" for k in STAT_KEYS if st[k] != ref.stats[k]]
        if any(st["nonfinite_px"]) or st["nonfinite_low_px"]:
            smsgs.append(f"a clean frame counted {st['nonfinite_px']} / {st['nonfinite_low_px']}")
        if st["calls"] != calls0 + 1:
            smsgs.append(f"calls rose by {st['calls'] - calls0}")
        stat_differs += bool(smsgs)
        bad += [f"{tag} {KIND[kind]} {MASK[mask]} {how} use {u}: {m}" for m in msgs]
        (bad if stat_bad is None else stat_bad).extend(f"{tag} {KIND[kind]} {MASK[mask]} {how} use {u}: {m}" for m in smsgs)
    en, inst, la = eng.dbg_slot_graphs()
    print(f"async_graph| {tag:<24} {KIND[kind]:<6} {MASK[mask]:<4} {how:<13} uses {uses} instantiated +{inst - inst0} launches +{la - la0} "
          f"enabled {en} differing {differing} tickets whose statistic differs {stat_differs}  infer_ms plain {ms[0]:.3f} replays {np.mean(ms[2:]):.3f}")
    if (inst - inst0, la - la0, en) != tuple(expect):
        bad.append(f"{tag} {KIND[kind]} {MASK[mask]} {how}: instantiated +{inst - inst0}, launches +{la - la0}, enabled {en}; expected "
                   f"+{expect[0]}, +{expect[1]}, {expect[2]}")
    return bad


def _held(eng, frame, ref):
    """a request that stays un-waited (tensor, both outputs) -> (request, finish); finish() waits it and returns its misses"""
    req = Req(eng, 0, frame, 3)

    def finish():
        req.wait()
        return [f"held ticket: {m}" for m in req.judge(ref.disp, ref.raw)[0]]
    return req, finish


def _call_list(eng, tag, frames, refs, expect=(1, 4, 1), stat_bad=None):
    """Every cell two slots can reach, each driven once through USES uses: slot 0 alone and slot 1 sharing for both kinds and
    the three masks, slot 0 sharing for both kinds with both outputs.  A held ticket is a further use of a cell that has been
    driven before (slot 0 alone / slot 1 sharing, tensor, both), outside the window the counts are read over.  -> misses"""
    bad = []
    cells = [(kind, mask) for kind in (0, 1) for mask in (3, 1, 2)]
    for kind, mask in cells:
        bad += _drive(eng, tag, kind, mask, "slot0 alone", frames, refs, expect, stat_bad=stat_bad)
    for kind, mask in cells:
        _, finish = _held(eng, frames[0][0], refs[0][0])                    # owns slot 0
        bad += _drive(eng, tag, kind, mask, "slot1 sharing", frames, refs, expect, stat_bad=stat_bad)
        bad += finish()
    for kind in (0, 1):
        a, finish_a = _held(eng, frames[0][1], refs[0][1])                  # slot 0
        _, finish_b = _held(eng, frames[0][2], refs[0][2])                  # slot 1, sharing
        bad += finish_a()                                                   # slot 0 is free, slot 1 owned
        bad += _drive(eng, tag, kind, 3, "slot0 sharing", frames, refs, expect, stat_bad=stat_bad)
        bad += finish_b()
    return bad


# ---- the share-size geometry ----------------------------------------------------------------------------------------------
def _streamed_launches(w, h, cus):
    """the schedule of every streamed tower launch of one pair at w x h with `cus` workgroups (tower_ref.stream_sched)"""
    wp, hp = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    out = [("f16", dil, tr.stream_sched(1, hp, wp, dil, tr.STREAM_OW_F16[dil], cus)) for dil in REF_DIL[:-1]]
    out.append(("f16 tail", 1, tr.stream_sched(1, h, w, 1, tr.STREAM_OW_TAIL, cus)))       # the tail form walks the output map
    return out + [("f16x3", dil, tr.stream_sched(1, hp, wp, dil, tr.STREAM_OW_X3[dil], cus)) for dil in REF_DIL]


def share_geometry(cus, w=64):
    """-> (w, h): the smallest even h at which every streamed launch of both towers gives its workgroups another number of
    rows with cus * 7 / 8 workgroups than with cus"""
    for h in range(16, 4096, 2):
        if all(a[2]["rpw"] != b[2]["rpw"] for a, b in zip(_streamed_launches(w, h, cus), _streamed_launches(w, h, cus * 7 // 8))):
            return w, h
    raise AssertionError(f"no share-size geometry for {cus} CUs")


def _num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


GEOMETRIES = {"96x64": lambda: (96, 64, 48, False), "124x38-padded": lambda: (124, 38, 32, False),
              "96x64-multi": lambda: (96, 64, 48, True), "share-size": lambda: (*share_geometry(_num_cu()), 32, False)}
PRECISIONS = [("f16", api.PREC_F16), ("f16x3", api.PREC_F16X3), ("fp32", api.PREC_FP32)]


def _check_share_grids(eng, w, h, cus):
    """the two grids of the first streamed block at the share-size geometry, on the device: the hook's launcher is the
    pipeline's, capped as submit_common caps a sharing request"""
    hp, wp = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    full = tr.stream_sched(1, hp, wp, 1, tr.STREAM_OW_F16[1], cus)
    share = tr.stream_sched(1, hp, wp, 1, tr.STREAM_OW_F16[1], cus * 7 // 8)
    blk = tr.random_block(1, hp, wp, 5, fp16=True)
    got = []
    for cap in (0, cus * 7 // 8):
        eng.dbg_set_grid_cus(cap)
        eng.dbg_ref_block_f16(blk[0][0], *blk[1:], dil=1, fused=2)
        got.append(eng.dbg_last_launch())
    eng.dbg_set_grid_cus(0)
    print(f"async_graph| share-size {w}x{h} on {cus} CUs: first streamed block {full['total']} rows, alone {full['grid']} workgroups x "
          f"{full['rpw']} rows, sharing {share['grid']} x {share['rpw']}; the device launched {got[0]} and {got[1]}")
    assert full["rpw"] != share["rpw"] and full["total"] > cus * 7 // 8
    assert got == [(full["grid"], full["total"]), (share["grid"], share["total"])], got


# ---- (a) every cell, (b) the statistic per ticket ---------------------------------------------------------------------------
_cells_done = {}


def _cells(model_factory, gname, pname, prec):
    """one handle of (geometry, forced precision) with two slots through `_call_list`, once per process
    -> (misses of the maps and the counts, misses of the statistic)"""
    if (gname, pname) not in _cells_done:
        w, h, d, multi = GEOMETRIES[gname]()
        tag = f"{w}x{h}{'m' if multi else ''} D{d} {pname}"
        frames = _frames(w, h, d)
        bad, stat_bad = [], []
        _cells_done[gname, pname] = (bad, stat_bad)
        with api.StereoNetHIP(model_factory(w, h, d, multi=multi), precision=prec, task_num=2) as eng:
            if gname == "share-size" and prec == api.PREC_F16:
                _check_share_grids(eng, w, h, _num_cu())
            refs = [[_sync_ref(eng, kind, f) for f in frames[kind]] for kind in (0, 1)]
            assert all(r.stats["precision_last"] == pname for rs in refs for r in rs)
            assert not _bits_differ(refs[0][0].raw, eng.infer(frames[0][0])[1])                    # the target is deterministic
            assert all(_bits_differ(refs[k][0].raw, refs[k][1].raw) for k in (0, 1))               # ... and tells frames apart
            assert eng.dbg_slot_graphs() == (1, 0, 0)
            bad += _call_list(eng, tag, frames, refs, stat_bad=stat_bad)
            en, inst, la = eng.dbg_slot_graphs()
            print(f"async_graph| {tag:<24} handle: enabled {en} instantiated {inst} launches {la}")
            if (en, inst) != (1, 14):
                bad.append(f"{tag}: enabled {en}, instantiated {inst} over 14 cells, launches {la}")
    return _cells_done[gname, pname]


@pytest.mark.parametrize("pname,prec", PRECISIONS)
@pytest.mark.parametrize("gname", list(GEOMETRIES))
def test_every_cell_replays_the_synchronous_call(model_factory, gname, pname, prec):
    """(a): per geometry and forced precision one handle with two slots through `_call_list`: 14 cells x 5 uses, every use
    another frame.  Every ticket: maps bit for bit the synchronous call's, guards intact, an unasked buffer unwritten.  Every
    cell: instantiated + 1, launches + 4, graphs still enabled.  SN_PREC_FP32 launches no streamed tower kernel, so its
    sharing cells run the alone cells' grids: covered for the cell bookkeeping all the same."""
    bad, _ = _cells(model_factory, gname, pname, prec)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("pname,prec", PRECISIONS)
@pytest.mark.parametrize("gname", list(GEOMETRIES))
def test_every_ticket_carries_the_synchronous_statistic(model_factory, gname, pname, prec):
    """(b): after each wait of (a), level_px / residual_px / nonfinite_px / nonfinite_low_px / precision_last equal to what the
    synchronous call of that frame left on the same handle, all counts zero, and calls + 1 per ticket.  Equality, as the sums
    are integer atomics; a difference is a finding, not a tolerance to choose.

    This check found one thing.  At 64x226 in SN_PREC_F16 a request that shared the GPU returned the synchronous call's maps
    bit for bit and a residual_px one unit of the 2^-20 px fixed point away from it on one or two frames of five
    (0.09031282444443323 against 0.09031282451036757: 6.6e-11 px): the tail form of the streamed block added its |D r| in
    fp32 per lane and wave and rounded to fixed point once per wave, so the total followed how ws.tower_cu cut the rows into
    shares (three rows a workgroup where the synchronous call has two).  The tail form now takes every pixel to fixed point
    before any addition (stat_fixed / refine_stat_commit_fixed, sn_kernels.hpp): integers from there on, the same total for
    every grid.  SN_PREC_F16X3 and SN_PREC_FP32 commit from a head launch of their own whose grid does not follow tower_cu."""
    _, stat_bad = _cells(model_factory, gname, pname, prec)
    assert not stat_bad, "\n".join(stat_bad)


# ---- (c) flags over one graph -----------------------------------------------------------------------------------------------
def test_flagged_tickets_over_one_graph(tmp_path):
    """(c): S-tower+16 and S-low+16 with F16 forced, alternating on two handles (no clean input exists under either model,
    see the module's docstring), each over slot 0's alone cell through six uses of three frames.  Every ticket raises
    StereoNetRangeError with the synchronous call's counts of its frame (a replay that accumulated would show the sum), its maps are the synchronous call's, its ticket is consumed and its slot is free again."""
    w, h, d = tc.SHAPE_S
    kinds = (tc.RANGE_INPUT, "noise", "step")
    xs = [tc.domain_input(w, h, d, k) for k in kinds]
    engs, refs, bad = {}, {}, []
    try:
        for name in ("S-tower+16", "S-low+16"):
            path = str(tmp_path / f"{name}.snw")
            weights.save_snw(path, tc.range_blob(name), w, h, d)
            engs[name] = eng = api.StereoNetHIP(path, precision=api.PREC_F16, task_num=2)
            refs[name] = []
            for x in xs:
                with pytest.raises(api.StereoNetRangeError) as e:
                    eng.infer(x)
                refs[name].append((e.value.outputs[0], e.value.outputs[1], list(e.value.nonfinite_px), e.value.nonfinite_low_px))
            counts = [(r[2], r[3]) for r in refs[name]]
            print(f"async_graph| flags {name}: synchronous counts per frame {counts}")
            assert all(any(c[0]) or c[1] for c in counts), counts
        for u in range(6):
            for name, eng in engs.items():
                disp, raw, px, low = refs[name][u % 3]
                req = Req(eng, 0, xs[u % 3], 3)
                req.wait()
                msgs = req.judge(disp, raw)[0]
                if req.flag is None:
                    msgs.append(f"returned SN_OK where the synchronous call counted {px} / {low}")
                elif (req.flag.nonfinite_px, req.flag.nonfinite_low_px) != (px, low):
                    msgs.append(f"counts {req.flag.nonfinite_px} / {req.flag.nonfinite_low_px}, the synchronous call's are {px} / {low}")
                with pytest.raises(api.StereoNetError) as e:
                    eng.wait(req.ticket)
                if e.value.code != SN_ERR_TICKET:
                    msgs.append(f"a second wait returned {e.value.code}")
                bad += [f"{name} use {u}: {m}" for m in msgs]
        for name, eng in engs.items():
            en, inst, la = eng.dbg_slot_graphs()
            print(f"async_graph| flags {name:<10} tensor both slot0 alone   uses 6 instantiated +{inst} launches +{la} enabled {en}")
            assert (en, inst, la) == (1, 1, 5), (name, en, inst, la)
            # a flagged wait frees its slot: both slots can be taken at once, and again
            for _ in range(2):
                pair = [Req(eng, 0, xs[0], 3), Req(eng, 0, xs[1], 3)]
                for req, ref in zip(pair, refs[name]):
                    req.wait()
                    bad += [f"{name} after the flags: {m}" for m in req.judge(ref[0], ref[1])[0]]
                    assert req.flag is not None and (req.flag.nonfinite_px, req.flag.nonfinite_low_px) == (ref[2], ref[3])
    finally:
        for eng in engs.values():
            eng.close()
    assert not bad, "\n".join(bad)


# ---- (d) AUTO across replays ------------------------------------------------------------------------------------------------
def test_the_default_precision_across_replays(tmp_path):
    """(d): the sequence rig's single-scale model on a handle of the default precision, one ticket at a time over slot 0's
    alone cells.  Five calm frames: the F16 cell is plain, captured, replayed.  `max` leaves the envelope: a replay of the
    F16 graph, repeated in F16X3 by sn_wait on the slot's workspace outside the graph — reruns + 1, the forced F16X3 maps.
    The tickets that follow are submitted in F16X3 and go through that cell's own plain, capture and replay uses.  Once the
    state machine is back in F16 the OLD F16 graph is replayed, after the repeat and the second self-check used the slot's
    workspace outside it: still the forced F16 maps.  Two graphs in all, every other request a launch of one of them."""
    model = "single"
    w, h, d = tc.SHAPE_S
    path = str(tmp_path / "seq.snw")
    weights.save_snw(path, tc.seq_blob(model), w, h, d)
    xs = {f: tc.seq_input(f) for f in tc.SEQ_CALM + ("max", "step")}
    forced = {}
    for mode, prec in (("f16", api.PREC_F16), ("f16x3", api.PREC_F16X3)):
        with api.StereoNetHIP(path, precision=prec) as eng:
            for f, x in xs.items():
                forced[f, mode] = eng.infer(x)
    bad, log = [], []

    def ticket(eng, f):
        start = api.PREC_NAMES[eng.precision_selected]
        reruns0 = eng.refine_stats()["reruns"]
        req = Req(eng, 0, xs[f], 3, TIMEOUT_MS)
        req.wait()
        st = eng.refine_stats()
        ran = st["precision_last"]
        msgs = req.judge(*forced[f, ran])[0] if ran in ("f16", "f16x3") else [f"ran {ran}"]
        if req.flag is not None:
            msgs.append(f"flagged: {req.flag}")
        if start == "f16x3" and ran != "f16x3":
            msgs.append(f"submitted in f16x3, returned in {ran}")
        if st["reruns"] - reruns0 != int(start == "f16" and ran == "f16x3"):
            msgs.append(f"submitted in {start}, returned in {ran}, reruns rose by {st['reruns'] - reruns0}")
        bad.extend(f"ticket {len(log)} ({f}, submitted in {start}): {m}" for m in msgs)
        log.append((f, start, ran))
        print(f"async_graph| auto ticket {len(log) - 1:2d} {f:<5} submitted in {start:<6} returned {ran:<6} residual {st['residual_px']:.4f} limit "
              f"{st['limit_px']:.4f} reruns {st['reruns']} switches {st['switches']} graphs {eng.dbg_slot_graphs()}")
        return start, ran

    with api.StereoNetHIP(path, task_num=2) as eng:
        assert eng.precision == api.PREC_AUTO
        for i in range(5):
            assert ticket(eng, tc.SEQ_CALM[i % 4]) == ("f16", "f16"), log[-1]
        assert eng.dbg_slot_graphs() == (1, 1, 4)                          # the F16 graph is being replayed
        assert ticket(eng, "max") == ("f16", "f16x3"), log[-1]             # ... and this one was a replay of it, then repeated
        assert eng.dbg_slot_graphs() == (1, 1, 5) and eng.refine_stats()["reruns"] == 1
        assert ticket(eng, "step")[0] == "f16x3", log[-1]
        n_x3 = 1
        for i in range(16):                                                # calm calls until the state machine re-enters F16
            if api.PREC_NAMES[eng.precision_selected] == "f16":
                break
            assert ticket(eng, tc.SEQ_CALM[i % 4]) == ("f16x3", "f16x3"), log[-1]
            n_x3 += 1
        assert api.PREC_NAMES[eng.precision_selected] == "f16", "the handle did not return to F16 within 16 calm tickets"
        assert n_x3 >= 3, n_x3                                             # the F16X3 cell was plain, captured and replayed
        assert eng.dbg_slot_graphs() == (1, 2, 5 + n_x3 - 1)
        for i in range(3):                                                 # the old F16 graph, after the repeat used the workspace
            assert ticket(eng, tc.SEQ_CALM[(i + 1) % 4]) == ("f16", "f16"), log[-1]
        en, inst, la = eng.dbg_slot_graphs()
        st = eng.refine_stats()
        print(f"async_graph| auto {w}x{h} D{d}: {len(log)} tickets, {n_x3} submitted in f16x3, enabled {en} instantiated {inst} launches {la} "
              f"reruns {st['reruns']} switches {st['switches']}")
        assert (en, inst, la) == (1, 2, len(log) - 2), (en, inst, la, len(log))
        assert st["calls"] == len(log) and st["reruns"] == 1 and st["switches"] >= 2, st
    assert not bad, "\n".join(bad)


# ---- (e) SN_NO_GRAPH --------------------------------------------------------------------------------------------------------
def test_sn_no_graph_equals_the_graph_handle(model_factory, monkeypatch):
    """(e): the switch is read at sn_create.  A handle made under SN_NO_GRAPH=1 goes through the call list of (a) at 96x64 in
    F16 with enabled / instantiated / launches all 0, and every map (and statistic) is the graph handle's: the references
    are the synchronous calls of a handle made without the switch, which also replays one cell here."""
    w, h, d = 96, 64, 48
    frames = _frames(w, h, d)
    path = model_factory(w, h, d)
    monkeypatch.delenv("SN_NO_GRAPH", raising=False)
    with api.StereoNetHIP(path, precision=api.PREC_F16, task_num=2) as graph:
        monkeypatch.setenv("SN_NO_GRAPH", "1")
        with api.StereoNetHIP(path, precision=api.PREC_F16, task_num=2) as plain:
            monkeypatch.delenv("SN_NO_GRAPH")
            refs = [[_sync_ref(graph, kind, f) for f in frames[kind]] for kind in (0, 1)]
            bad = _drive(graph, "96x64 D48 f16 graphs on", 0, 3, "slot0 alone", frames, refs)
            assert plain.dbg_slot_graphs() == (0, 0, 0)
            for kind in (0, 1):                                  # the plain handle's own synchronous calls agree too
                got = _sync_ref(plain, kind, frames[kind][0])
                assert not _bits_differ(got.raw, refs[kind][0].raw) and not _bits_differ(got.disp, refs[kind][0].disp)
            bad += _call_list(plain, "96x64 D48 f16 SN_NO_GRAPH", frames, refs, expect=(0, 0, 0))
            print(f"async_graph| 96x64 D48 f16 SN_NO_GRAPH handle: enabled / instantiated / launches {plain.dbg_slot_graphs()}; "
                  f"graph handle {graph.dbg_slot_graphs()}")
            assert plain.dbg_slot_graphs() == (0, 0, 0) and graph.dbg_slot_graphs() == (1, 1, 4)
    assert not bad, "\n".join(bad)


# ---- (f) other work between replays -----------------------------------------------------------------------------------------
def test_other_work_between_replays(model_factory):
    """(f): between two replays of one cell a synchronous batch on the handle's own workspace and an enqueue-only
    infer_device on a caller's stream: the next replay is its frame's map, and the synchronous results are theirs."""
    import torch
    w, h, d = 96, 64, 48
    frames = _frames(w, h, d, n=6)
    batch = np.stack(frames[0][3:6])
    stream = torch.cuda.Stream()
    dx = torch.from_numpy(batch).cuda()
    draw = torch.empty((3, h, w), dtype=torch.int32, device="cuda")
    ddisp = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with api.StereoNetHIP(model_factory(w, h, d), precision=api.PREC_F16, max_batch=3, task_num=2) as eng:
        refs = [[_sync_ref(eng, 0, f) for f in frames[0]], []]
        bad = _drive(eng, "96x64 D48 f16 (f)", 0, 3, "slot0 alone", frames, refs, uses=3, expect=(1, 2, 1))
        for rep in range(2):
            disp, raw = eng.infer(batch)
            eng.infer_device(3, dx.data_ptr(), draw.data_ptr(), ddisp.data_ptr(), stream.cuda_stream)
            req = Req(eng, 0, frames[0][rep], 3)                       # a replay, submitted while the caller's stream may still run
            req.wait()
            bad += [f"replay {rep} after other work: {m}" for m in req.judge(refs[0][rep].disp, refs[0][rep].raw)[0]]
            stream.synchronize()
            eng.synchronize()
            for i in range(3):
                r = refs[0][3 + i]
                if _bits_differ(raw[i], r.raw) or _bits_differ(disp[i], r.disp):
                    bad.append(f"rep {rep}: pair {i} of the synchronous batch differs from its single call")
                if _bits_differ(draw[i].cpu().numpy(), r.raw) or _bits_differ(ddisp[i].cpu().numpy(), r.disp):
                    bad.append(f"rep {rep}: pair {i} of the enqueue-only call differs from its single call")
            draw.zero_()
            ddisp.zero_()
            torch.cuda.synchronize()
        en, inst, la = eng.dbg_slot_graphs()
        print(f"async_graph| 96x64 D48 f16 other work between replays: enabled {en} instantiated {inst} launches {la}")
        assert (en, inst, la) == (1, 1, 4)
    assert not bad, "\n".join(bad)


# ---- (g) two threads on one handle ------------------------------------------------------------------------------------------
def test_two_threads_on_one_handle(model_factory):
    """(g): task_num = 4, two threads, 12 tickets each of their own frames, submit and wait in turn: captures in one thread run
    while the other waits and copies.  Every map is its frame's synchronous map; the graphs served requests and stayed on."""
    w, h, d = 96, 64, 48
    frames = _frames(w, h, d, n=6)
    bad = []
    with api.StereoNetHIP(model_factory(w, h, d), precision=api.PREC_F16, task_num=4) as eng:
        refs = [_sync_ref(eng, 0, f) for f in frames[0]]

        def work(first):
            try:
                for i in range(12):
                    k = first + i % 3
                    req = Req(eng, 0, frames[0][k], 3)
                    req.wait()
                    bad.extend(f"thread {first // 3} ticket {i}: {m}" for m in req.judge(refs[k].disp, refs[k].raw)[0])
            except Exception as e:                        # noqa: BLE001 - reported by the main thread
                bad.append(f"thread {first // 3}: {e!r}")

        threads = [threading.Thread(target=work, args=(first,), daemon=True) for first in (0, 3)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(60)
        assert not any(t.is_alive() for t in threads), "a thread did not finish its 12 tickets"
        en, inst, la = eng.dbg_slot_graphs()
        print(f"async_graph| 96x64 D48 f16 two threads x 12 tickets: enabled {en} instantiated {inst} launches {la}")
        assert en == 1 and la > 0 and inst >= 1, (en, inst, la)
        assert eng.refine_stats()["calls"] == 6 + 24
    assert not bad, "\n".join(bad)


# ---- the slot protocol ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def proto(model_factory):
    """(frames, the synchronous maps of every frame, the model file) at 96x64 in F16"""
    w, h, d = 96, 64, 48
    frames = _frames(w, h, d, n=6)
    path = model_factory(w, h, d)
    with api.StereoNetHIP(path, precision=api.PREC_F16) as eng:
        refs = [_sync_ref(eng, 0, f) for f in frames[0]]
    return frames, refs, path


def _raw_submit(eng, frame, raw, disp, timeout_ms, nv12_size=None):
    """sn_submit / sn_submit_nv12 below the binding -> (return code, the ticket word, which held 0xDEAD before the call)"""
    t = C.c_uint64(0xDEAD)
    if nv12_size is None:
        rc = eng._lib.sn_submit(eng._h, frame.ctypes.data, raw.view.ctypes.data, disp.view.ctypes.data, timeout_ms, C.byref(t))
    else:
        rc = eng._lib.sn_submit_nv12(eng._h, frame.ctypes.data, nv12_size[0], nv12_size[1], raw.view.ctypes.data, disp.view.ctypes.data,
                                     timeout_ms, C.byref(t))
    return rc, t.value


def _finish(req, ref, what):
    req.wait()
    return [f"{what}: {m}" for m in req.judge(ref.disp, ref.raw)[0]]


def test_busy_and_the_slot_a_wait_frees(proto):
    """Two slots, two un-waited tickets: a submit with timeout 0 and one with 50 ms return SN_ERR_BUSY and write neither the
    ticket nor the outputs.  After one wait the next submit takes the slot that was freed, read from the cell it lands in:
      wait t2 (slot 1) -> slot 1 sharing, that cell's second use: a capture (instantiated 1, launches 1);
      wait t1 (slot 0), slot 1 owned -> slot 0 SHARING, first use: plain (still 1 / 1; slot 0 alone would have captured);
      everything waited -> slot 0 alone, second use: a capture (2 / 2)."""
    frames, refs, path = proto
    f = frames[0]
    with api.StereoNetHIP(path, precision=api.PREC_F16, task_num=2) as eng:
        t1, t2 = Req(eng, 0, f[0], 3), Req(eng, 0, f[1], 3)
        assert eng.dbg_slot_graphs() == (1, 0, 0)
        for timeout in (0, 50):
            raw, disp = Out(eng.height, eng.width, np.int32), Out(eng.height, eng.width, np.float32)
            rc, word = _raw_submit(eng, f[2], raw, disp, timeout)
            assert rc == SN_ERR_BUSY and word == 0xDEAD, (timeout, rc, word)
            assert raw.untouched() and disp.untouched()
            with pytest.raises(api.StereoNetError) as e:
                eng.submit(f[2], raw.view, disp.view, timeout_ms=timeout)
            assert e.value.code == SN_ERR_BUSY
        assert eng.dbg_slot_graphs() == (1, 0, 0)
        bad = _finish(t2, refs[1], "t2")
        t3 = Req(eng, 0, f[2], 3)
        assert eng.dbg_slot_graphs() == (1, 1, 1), eng.dbg_slot_graphs()
        bad += _finish(t1, refs[0], "t1")
        t4 = Req(eng, 0, f[3], 3)
        assert eng.dbg_slot_graphs() == (1, 1, 1), eng.dbg_slot_graphs()
        bad += _finish(t3, refs[2], "t3") + _finish(t4, refs[3], "t4")
        t5 = Req(eng, 0, f[4], 3)
        assert eng.dbg_slot_graphs() == (1, 2, 2), eng.dbg_slot_graphs()
        bad += _finish(t5, refs[4], "t5")
    assert not bad, "\n".join(bad)


def test_waits_in_reverse_order_and_spent_tickets(proto):
    """Four tickets waited last first: each returns its own frame's maps.  A second wait on a ticket is SN_ERR_TICKET, wait(0)
    SN_ERR_ARG."""
    frames, refs, path = proto
    bad = []
    with api.StereoNetHIP(path, precision=api.PREC_F16, task_num=4) as eng:
        for rep in range(3):                                         # plain, capture, replay in all four slots
            reqs = [Req(eng, 0, frames[0][(i + rep) % 6], 3) for i in range(4)]
            for i in reversed(range(4)):
                bad += _finish(reqs[i], refs[(i + rep) % 6], f"round {rep} ticket {i}")
        for req in reqs:
            with pytest.raises(api.StereoNetError) as e:
                eng.wait(req.ticket)
            assert e.value.code == SN_ERR_TICKET
        with pytest.raises(api.StereoNetError) as e:
            eng.wait(0)
        assert e.value.code == SN_ERR_ARG
        assert eng.dbg_slot_graphs() == (1, 4, 8)
    assert not bad, "\n".join(bad)


def test_error_exits_hand_the_slot_back(proto):
    """After a submit with both outputs None, a submit_nv12 with a wrong frame size and a submit that timed out, task_num
    further submits succeed without SN_ERR_BUSY (finite timeout) and return their frames' maps."""
    frames, refs, path = proto
    bad = []
    with api.StereoNetHIP(path, precision=api.PREC_F16, task_num=2) as eng:
        w, h = eng.width, eng.height

        def both_slots_work(what):
            reqs = [Req(eng, 0, frames[0][i], 3) for i in range(2)]
            return [m for i, r in enumerate(reqs) for m in _finish(r, refs[i], f"after {what}, ticket {i}")]

        for rep in range(2):
            with pytest.raises(api.StereoNetError) as e:
                eng.submit(frames[0][0], None, None, timeout_ms=TIMEOUT_MS)
            assert e.value.code == SN_ERR_ARG
            bad += both_slots_work("a submit without outputs")
            raw, disp = Out(h, w, np.int32), Out(h, w, np.float32)
            for size in ((2 * w, h + 2), (2 * w + 8, h)):
                rc, word = _raw_submit(eng, frames[1][0], raw, disp, TIMEOUT_MS, nv12_size=size)
                assert rc == SN_ERR_ARG and word == 0xDEAD and raw.untouched() and disp.untouched(), (size, rc, word)
            bad += both_slots_work("a submit_nv12 of a wrong size")
            held = [Req(eng, 0, frames[0][i], 3) for i in range(2)]
            with pytest.raises(api.StereoNetError) as e:
                eng.submit(frames[0][2], raw.view, disp.view, timeout_ms=20)
            assert e.value.code == SN_ERR_BUSY and raw.untouched() and disp.untouched()
            for i, r in enumerate(held):
                bad += _finish(r, refs[i], f"held ticket {i}")
            bad += both_slots_work("a submit that timed out")
    assert not bad, "\n".join(bad)


def test_a_blocked_submit_is_released_by_a_wait(proto):
    """All slots owned; a second thread calls submit(timeout_ms = 20000).  After 0.2 s it has not returned; the main thread
    waits the oldest ticket, the submit comes back with a ticket, and its maps are its frame's."""
    frames, refs, path = proto
    with api.StereoNetHIP(path, precision=api.PREC_F16, task_num=2) as eng:
        held = [Req(eng, 0, frames[0][i], 3) for i in range(2)]
        got = {}

        def blocked():
            try:
                got["req"] = Req(eng, 0, frames[0][2], 3, TIMEOUT_MS)
            except Exception as e:                        # noqa: BLE001 - reported by the main thread
                got["error"] = e

        t = threading.Thread(target=blocked, daemon=True)
        t.start()
        time.sleep(0.2)
        assert t.is_alive() and not got, "the submit returned while every slot was owned"
        bad = _finish(held[0], refs[0], "oldest ticket")
        t.join(30)
        assert not t.is_alive(), "the blocked submit was not released by the wait"
        assert "req" in got, got
        bad += _finish(got["req"], refs[2], "the released submit") + _finish(held[1], refs[1], "second ticket")
    assert not bad, "\n".join(bad)
