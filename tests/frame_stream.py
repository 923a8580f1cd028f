"""Helpers for the frame-stream tests (test_frame_stream_cpu.py, test_frame_stream_gpu.py): a scripted stream of sort events and
asynchronous frames, the model of which events a frame may read, the stream runner and the serial replay it is compared with.

The image of frame k is a pure function of (camera_k, scene uniforms_k, draw list of event j).  Timing decides which j a frame of an
asynchronous stream reads; the options fix the small window of j it MAY read (allowed_events).  The replay sets one event at a time,
waits, and renders with synchronous calls every frame whose window holds that event; each streamed frame then has to equal one of
its window's replay images bit for bit, with the matched event never going back (match_stream).  A half-built list, the list of a
set that was refilled under the frame, or a stale one matches nothing."""
from __future__ import annotations

import functools

import numpy as np

from gswt_renderer_amd import _lib as L
from gswt_renderer_amd import host, synth

# the scene of the merged-group reuse tests (tests/test_end_to_end_gpu.py)
CFG = dict(tile_map_half_wh=(4, 4), surface_type=0, lod_max_dist=22.0, tile_sort_type=host.SORT_GRAPH, merge_type=host.MERGE_EDGE,
           merge_topk=40, lod_blending=True)
W, HH = 320, 200
T_EPS = 1e-5
DEFAULT_SLOTS = 5                 # GSWT_FRAME_SLOTS of csrc/gswt_ctx.h; the GPU tests ask the library (frame_slots())
SOURCES = ("host", "merge", "rows", "worker")

# three viewing directions at one place (the tile map stays, the merged groups and their presort views change) ...
PLACES = [((4.2, 1.0, 1.5), (5.0, 4.0, 1.0)), ((4.3, 1.1, 1.5), (8.0, 0.5, 1.0)), ((4.1, 0.9, 1.5), (1.0, 3.5, 1.0))]


def crossing(k):
    """... and a path that crosses a cell border every other step (tile_width 4): the tile map is rebuilt, center_coord moves."""
    return (4.25 + 2.3 * k, 1.05 + 1.1 * k, 1.5), (5.0 + 2.3 * k, 4.0 + 1.3 * k, 1.0)


def _look(cam, i):
    """The i-th frame camera after an event at cam: the same position, the target nudged (every frame has its own image)."""
    (pos, tgt) = cam
    return pos, (tgt[0] + 0.11 * (i + 1), tgt[1] - 0.07 * (i + 1), tgt[2] + 0.02 * i)


@functools.lru_cache(maxsize=4)
def make_schedule(slots: int = DEFAULT_SLOTS):
    """The scripted stream: a tuple of ("event", cam), ("frame", cam) and ("sync",) steps, cam = (position, target).  In order:

    1. events every third frame along `crossing`: four events, each followed by three frames; the path crosses cell borders, so at
       least two of these events rebuild the tile map and change center_coord (the scene uniforms a frame gets are those of the
       newest event, whichever list it ends up reading);
    2. the three PLACES round robin, three laps, an event every third frame: from the second lap on every merged group is copied
       from a draw set two or three events back while those sets rotate;
    3. two events with no frame between them, then two frames;
    4. a ("sync",), then one frame: it must read the newest event;
    5. `slots` frames with no event, so that every slot holds an uncollected frame, and an event directly after them;
    6. `slots` times (event, frame): the `slots` frames in flight now each read another draw set -- then a burst of `slots` + 7
       events with no frame in between: the ring of slots + 5 draw sets wraps onto the sets those frames still read;
    7. four frames, an event back on the crossing path (another rebuild), three frames.

    Frames are collected only when every slot is taken, oldest first (run_stream), so from the `slots`-th frame on every event
    meets `slots` uncollected frames.  A frame looks from the place of the newest event: the draw list of an event holds the tiles its
    own camera sees, so on its own event's list every frame has more than 4096 (tile, splat) pairs, and the lists of two events in
    a row never give a frame the same image (tests/test_frame_stream_cpu.py holds the schedule's other promises)."""
    s = []

    def event(cam):
        s.append(("event", cam))

    def frames(cam, n):
        for i in range(n):
            s.append(("frame", _look(cam, i)))

    for k in range(4):                                   # 1
        event(crossing(k)); frames(crossing(k), 3)
    for k in range(9):                                   # 2
        event(PLACES[k % 3]); frames(PLACES[k % 3], 3)
    event(PLACES[0]); event(crossing(1)); frames(crossing(1), 2)      # 3
    s.append(("sync",)); frames(crossing(1), 1)          # 4
    frames(crossing(1), slots); event(PLACES[2])         # 5
    for k in range(slots):                               # 6
        cam = PLACES[k % 3] if k % 2 == 0 else crossing(k % 3)
        event(cam); frames(cam, 1)
    for k in range(slots + 7):
        event(PLACES[k % 3] if k % 4 != 3 else crossing(k % 3))
    last = PLACES[(slots + 6) % 3] if (slots + 6) % 4 != 3 else crossing((slots + 6) % 3)
    frames(last, 4)                                      # 7
    event(crossing(3)); frames(crossing(3), 3)
    return tuple(s)


def burst_length(schedule):
    """The longest run of events with no frame in between."""
    best = run = 0
    for st in schedule:
        if st[0] == "event":
            run += 1
            best = max(best, run)
        elif st[0] == "frame":
            run = 0
    return best


def event_cams(schedule):
    return [st[1] for st in schedule if st[0] == "event"]


def frame_cams(schedule):
    return [st[1] for st in schedule if st[0] == "frame"]


def newest_events(schedule):
    """n_k of every frame: the index of the newest event set before the frame was submitted."""
    n, out = -1, []
    for st in schedule:
        if st[0] == "event":
            n += 1
        elif st[0] == "frame":
            assert n >= 0, "a frame before the first event"
            out.append(n)
    return out


def allowed_events(schedule, defer):
    """The window of every frame: a list, per frame in submission order, of the sorted event indices whose draw list the frame may
    have read under GSWT_OPT_DEFER_SWAP = defer.  Restated from the rule the library documents, not taken from it:

    0: the newest event, n_k.
    1: a new list is read from the first frame submitted after its build has finished; until then frames keep the previous one,
       and the next event makes a list that is still waiting current.  So {n_k - 1, n_k}; only n_k when it is the first event
       (nothing to keep) or when a synchronize() lies between the event and the frame.
    n >= 2: no timing in it.  The first n - 1 frames submitted after an event's call read the list that was current at the call,
       the n-th and later ones read the new list; a following event makes the waiting list current at once and restarts the count."""
    out = []
    cur, pend, left, n = None, None, 0, -1
    for st in schedule:
        if st[0] == "event":
            n += 1
            if defer == 0 or cur is None:
                cur, pend = n, None
            else:
                if pend is not None:
                    cur = pend
                pend, left = n, defer - 1
        elif st[0] == "sync":
            if defer == 1 and pend is not None:
                cur, pend = pend, None
        else:
            assert cur is not None, "a frame before the first event"
            if defer >= 2 and pend is not None:
                if left <= 0:
                    cur, pend = pend, None
                else:
                    left -= 1
            out.append(sorted({cur} | ({pend} if defer == 1 and pend is not None else set())))
    return out


def camera(cam):
    """(camera uniforms, view_proj) of cam = (position, target) at the frame size."""
    return host.camera_uniforms(cam[0], cam[1], (0, 0, 1), 45.0, 0.1, 2400.0, W, HH)


@functools.lru_cache(maxsize=1)
def tileset_vertices():
    return synth.make_tileset(n_lod=3, n_tile=16, lod0_count=900)


def host_events(cams):
    """host.WangTile alone (no GPU) through the events at `cams`: per event (rebuilt, center_coord, bytes of the scene uniforms,
    bytes of the draw list with the merged lists behind it)."""
    wang = host.WangTile(host.TileSet.from_vertices(tileset_vertices()))
    wang.configure(host.user_data(**CFG))
    out = []
    for cam in cams:
        _, vp = camera(cam)
        rebuilt = wang.check_update(cam[0])
        if rebuilt:
            wang.build_tiles(cam[0])
        s = wang.sort_tiles(cam[0], vp)
        su = wang.scene_uniforms()
        lst = b"".join(bytes(d) for d in s.draws) + s.merged_gs_index.tobytes() + s.merged_map_id.tobytes() + s.merged_lod_id.tobytes()
        out.append((bool(rebuilt), tuple(su.center_coord[:]), bytes(su), lst))
    wang.close()
    return out


class EventSource:
    """One way of producing sort events on a renderer: a fresh worker state and a fresh scene upload, then set(cam) per event.
    "host": GSWTPipeline.update with the merged lists from the host (gswt_set_draws); "merge": device_merge=True
    (gswt_set_draws_merge_groups); "rows": device_preprocess=True; "worker": DeviceWorker build_tiles / sort_tiles / swap_in()
    (gswt_set_draws_from_worker).  A fresh source reproduces the same tile maps, so two of them stepped through the same cameras
    set the same draw lists."""

    def __init__(self, renderer, source):
        from gswt_renderer_amd.pipeline import GSWTPipeline
        assert source in SOURCES, source
        self.source = source
        self.pipe = GSWTPipeline(tileset_vertices(), host.user_data(**CFG), renderer=renderer,
                                 device_merge=source in ("merge", "worker"), device_preprocess=source == "rows")
        self.wang = self.pipe.wang
        self.dev = None
        if source == "worker":
            from gswt_renderer_amd.worker import DeviceWorker
            self.dev = DeviceWorker(renderer, self.wang)

    def build(self, cam):
        """The worker's half of an event up to the sort (tile map on the host, handed to the device worker)."""
        pos = cam[0]
        if self.wang.check_update(pos) or self.wang.scene_data is None:
            self.wang.build_tiles(pos)
            self.dev.build_tiles(pos)

    def set(self, cam):
        """One sort event at cam, swapped in; -> the scene uniforms that belong to it."""
        _, vp = camera(cam)
        if self.dev is None:
            self.pipe.update(cam[0], vp, force_sort=True)
        else:
            self.build(cam)
            self.dev.sort_tiles(cam[0], vp)
            self.dev.swap_in()
        return self.wang.scene_uniforms()

    def close(self):
        if self.dev is not None:
            self.dev.close()
            self.dev = None


def _stats(renderer):
    built, reused = renderer.merge_stats()
    return dict(built=built, reused=reused, deep=renderer.merge_stats_deep(), graph=renderer.graph_stats())


class Stream:
    """What run_stream returns: images[k] (host arrays), frames[k] = (camera uniforms, scene uniforms, n_k), n_pairs[k] (the pair
    count the library reported when frame k was collected) and the merge / graph counters the stream added."""


def run_stream(renderer, source, schedule, *, order_mode=L.GSWT_ORDER_REFERENCE, pin_pair_cap=0, **options):
    """The schedule as an asynchronous stream on `renderer` under renderer.options(**options): events through a fresh EventSource,
    frames through render_async with the scene uniforms of the newest event, collected (render_wait, then copied to the host) only
    when every slot is taken, oldest first, and at the end.  pin_pair_cap > 0: GSWT_OPT_PAIR_CAP is set to it again in front of every
    frame (the library lets go of the pin once a frame has overflowed it), so that every frame overflows and is re-run when it is
    collected."""
    import torch
    slots = renderer.frame_slots()
    n_frames = sum(1 for st in schedule if st[0] == "frame")
    out = Stream()
    out.images, out.frames, out.n_pairs = [None] * n_frames, [], [None] * n_frames
    if pin_pair_cap:
        options = dict(options, PAIR_CAP=pin_pair_cap)
    with renderer.options(**options):
        src = EventSource(renderer, source)
        tickets = []                              # (ticket, frame index), oldest first
        try:
            bufs = [torch.zeros((HH, W, 4), dtype=torch.float32, device="cuda") for _ in range(n_frames)]
            torch.cuda.synchronize()              # the zero fills ran on torch's stream, the frames run on the slots' streams
            s0 = _stats(renderer)

            def collect():
                t, k = tickets.pop(0)
                renderer.render_wait(t)
                out.n_pairs[k] = renderer.timings()["n_pairs"]
                out.images[k] = bufs[k].cpu().numpy()

            su, n = None, -1
            for st in schedule:
                if st[0] == "event":
                    su = src.set(st[1])
                    n += 1
                elif st[0] == "sync":
                    renderer.synchronize()
                else:
                    cu, _ = camera(st[1])
                    if len(tickets) == slots:
                        collect()
                    k = len(out.frames)
                    if pin_pair_cap:
                        renderer.set_option(L.GSWT_OPT_PAIR_CAP, pin_pair_cap)
                    t = renderer.render_async(cu, su, W, HH, bufs[k].data_ptr(), transmittance_eps=T_EPS, order_mode=order_mode)
                    tickets.append((t, k))
                    out.frames.append((cu, su, n))
            while tickets:
                collect()
            renderer.synchronize()
            s1 = _stats(renderer)
        finally:
            for t, _ in tickets:                  # (a failure above: no ticket stays behind on the renderer)
                renderer.render_wait(t)
            renderer.synchronize()
            src.close()
    out.reused, out.deep = s1["reused"] - s0["reused"], s1["deep"] - s0["deep"]
    out.graph_launches = s1["graph"][0] - s0["graph"][0]
    return out


class Replay(dict):
    """{(k, j): image}; stats[(k, j)] = (n_visible, n_pairs) of that synchronous frame."""


def replay(renderer, source, needed, *, cams, order_mode=L.GSWT_ORDER_REFERENCE):
    """The serial reading of a stream: a fresh EventSource stepped through the events at `cams`, one at a time, with
    DEFER_SWAP = 0, GRAPH = 0 and NO_MERGE_REUSE = 1 -- every list sorted anew, nothing copied, nothing deferred, nothing in flight.
    After event j and a synchronize(), every (k, j) of `needed` is rendered with the synchronous call.
    needed: {(k, j): (camera uniforms, scene uniforms)} -- frame k's own camera and scene uniforms, whatever event j is."""
    by_event = {}
    for (k, j), v in needed.items():
        by_event.setdefault(j, []).append((k, v))
    out = Replay()
    out.stats = {}
    with renderer.options(DEFER_SWAP=0, GRAPH=0, NO_MERGE_REUSE=1, PAIR_CAP=0):
        src = EventSource(renderer, source)
        try:
            for j, cam in enumerate(cams):
                if j > max(by_event):
                    break
                src.set(cam)
                renderer.synchronize()
                for k, (cu, su) in sorted(by_event.get(j, []), key=lambda e: e[0]):
                    out[(k, j)] = renderer.render(cu, su, W, HH, transmittance_eps=T_EPS, order_mode=order_mode)
                    t = renderer.timings()
                    out.stats[(k, j)] = (t["n_visible"], t["n_pairs"])
        finally:
            renderer.synchronize()
            src.close()
    return out


def match_stream(images, windows, rep):
    """The event each streamed frame read: per frame the smallest j of its window, not below the previous frame's, whose replay
    image equals the frame bit for bit.  Raises AssertionError for a frame that equals none (naming the frame, its window and how
    far it is from each candidate) -- also when it only equals a list older than one an earlier frame has already read."""
    matched, last = [], -1
    for k, (img, win) in enumerate(zip(images, windows)):
        equal = [j for j in win if np.array_equal(img, rep[(k, j)])]
        ok = [j for j in equal if j >= last]
        if not ok:
            far = {j: float(np.max(np.abs(img.astype(np.float64) - rep[(k, j)].astype(np.float64)))) for j in win}
            raise AssertionError(f"frame {k}: window {win}, equal to {equal}, previous frame read event {last}; max |diff| per event {far}")
        last = ok[0]
        matched.append(last)
    return matched


def needed_frames(frames, windows):
    """{(k, j): (camera uniforms, scene uniforms)} over the windows, for replay()."""
    return {(k, j): (cu, su) for k, ((cu, su, _), win) in enumerate(zip(frames, windows)) for j in win}


def schedule_frames(schedule, events=None):
    """frames[k] = (camera uniforms, scene uniforms, n_k) of the schedule without a GPU: the scene uniforms are those host.WangTile
    gives for event n_k (the event sources hold the same WangTile)."""
    events = events or host_events(event_cams(schedule))
    out = []
    for cam, n in zip(frame_cams(schedule), newest_events(schedule)):
        su = L.SceneUniforms.from_buffer_copy(events[n][2])
        out.append((camera(cam)[0], su, n))
    return out
