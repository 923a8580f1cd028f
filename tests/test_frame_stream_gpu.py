"""Every frame of an asynchronous frame stream across sort-event swap-ins (tests/frame_stream.py): frame_slots() frames in flight,
events from each of the four sources beside them, deferred swap-ins, the graph, merged lists copied on the device from draw sets
several events back, frames re-run after a pair overflow, and a worker on a second host thread.  Timing decides which event a
frame reads; what it MAY read is fixed, so every streamed frame must equal, bit for bit, the synchronous frame of a serial replay
for one event of its window, and the events matched must never go back.  The replay runs the same library, so three of its
frames per event source are held against the oracle at the project's image tolerance."""
import threading
import time

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from tests import frame_stream as FS
from tests import helpers as H

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # the project's image tolerance against the oracle (tests/test_end_to_end_gpu.py)
DEFERS = (0, 1, 3)


@pytest.fixture(scope="module")
def plan(renderer):
    """The schedule for this library's slot count, its frames (camera, scene uniforms, n_k), its windows per DEFER_SWAP value, and
    the replays: (source, order mode) -> Replay over the windows of every DEFER_SWAP value, each computed once by the first test that
    needs it (_replay) and only read afterwards."""
    sched = FS.make_schedule(renderer.frame_slots())
    frames = FS.schedule_frames(sched)
    windows = {d: FS.allowed_events(sched, d) for d in DEFERS}
    union = [sorted(set().union(*(windows[d][k] for d in DEFERS))) for k in range(len(frames))]
    p = dict(sched=sched, frames=frames, windows=windows, needed=FS.needed_frames(frames, union), cams=FS.event_cams(sched), replays={})
    yield p
    p["replays"].clear()


def _replay(renderer, plan, source, order_mode=L.GSWT_ORDER_REFERENCE):
    key = (source, order_mode)
    if key not in plan["replays"]:
        plan["replays"][key] = FS.replay(renderer, source, plan["needed"], cams=plan["cams"], order_mode=order_mode)
    return plan["replays"][key]


def _check_frames_are_the_schedules(stream, plan):
    """The stream handed the frames the cameras and scene uniforms the replay was rendered with."""
    assert len(stream.frames) == len(plan["frames"])
    for k, ((cu, su, n), (cu_p, su_p, n_p)) in enumerate(zip(stream.frames, plan["frames"])):
        assert n == n_p and bytes(cu) == bytes(cu_p) and bytes(su) == bytes(su_p), k


CASES = [(s, d, g, L.GSWT_ORDER_REFERENCE) for s in FS.SOURCES for d in DEFERS for g in (0, 1)]
CASES += [("merge", 1, g, L.GSWT_ORDER_DEPTH) for g in (0, 1)]


@pytest.mark.parametrize("source,defer,graph,order", CASES,
                         ids=[f"{s}-defer{d}-graph{g}-{'depth' if o else 'reference'}" for s, d, g, o in CASES])
def test_stream_matches_serial_replay(renderer, plan, source, defer, graph, order):
    rep = _replay(renderer, plan, source, order)
    stream = FS.run_stream(renderer, source, plan["sched"], order_mode=order, TIMING=0, GRAPH=graph, DEFER_SWAP=defer, PAIR_CAP=0,
                           NO_MERGE_REUSE=0)
    _check_frames_are_the_schedules(stream, plan)
    matched = FS.match_stream(stream.images, plan["windows"][defer], rep)
    assert matched == sorted(matched)
    early = sum(m < n for m, (_, _, n) in zip(matched, stream.frames))
    print(f"{source} defer {defer} graph {graph} order {order}: {len(matched)} frames checked, {len(set(matched))} distinct events read, "
          f"{early} frames on the list before the newest, groups copied {stream.reused} (from older events {stream.deep}), "
          f"graph launches {stream.graph_launches}")
    assert len(set(matched)) >= 10                          # the events are told apart by their images
    if source != "host":                                     # the copy path ran under frames in flight
        assert stream.reused > 0 and stream.deep > 0, (stream.reused, stream.deep)
    if graph:
        assert stream.graph_launches >= len(matched)
    else:
        assert stream.graph_launches == 0
    renderer.synchronize()


@pytest.mark.parametrize("defer", [0, 1])
def test_overflowing_frames_finish_on_their_own_list(renderer, plan, defer):
    """GSWT_OPT_PAIR_CAP pinned at 4096 in front of every frame: each one overflows its pair buffers and is re-run, against the draw
    set it was submitted with, when it is collected -- by then later events have been set and the burst has asked for its set back."""
    rep = _replay(renderer, plan, "merge")
    # on the newest event's list every frame of the schedule overflows the pinned capacity (one that keeps the list before it sees
    # fewer of that list's tiles and may not)
    assert min(rep.stats[(k, n)][1] for k, (_, _, n) in enumerate(plan["frames"])) > 4096
    stream = FS.run_stream(renderer, "merge", plan["sched"], pin_pair_cap=4096, TIMING=0, GRAPH=0, DEFER_SWAP=defer, NO_MERGE_REUSE=0)
    _check_frames_are_the_schedules(stream, plan)
    matched = FS.match_stream(stream.images, plan["windows"][defer], rep)
    assert matched == sorted(matched)
    for k, j in enumerate(matched):
        assert stream.n_pairs[k] == rep.stats[(k, j)][1], (k, j, stream.n_pairs[k], rep.stats[(k, j)])
    over = sum(p > 4096 for p in stream.n_pairs)
    print(f"overflow defer {defer}: {len(matched)} frames checked, {over} of them re-run, {len(set(matched))} distinct events read, "
          f"pairs per frame {min(stream.n_pairs)}..{max(stream.n_pairs)}")
    # (with the swap-in deferred a frame that keeps the list before the newest sees fewer of that list's tiles and may stay below)
    assert over >= sum(len(w) == 1 for w in plan["windows"][defer])
    renderer.synchronize()


ANCHORS = (0, 2, 4)             # events: the first one, one after a rebuild that moved center_coord, one more


@pytest.fixture(scope="module")
def oracle_frames(plan):
    """The oracle stepped through the first events of the schedule (as tests/test_end_to_end_gpu.py steps it): for each anchor event j
    the first frame k with n_k = j, rendered by the oracle -> {(k, j): (image, stats)}."""
    from oracle import gswt_oracle as orc
    from oracle import wangtile_oracle as wo
    verts = FS.tileset_vertices()
    pp = orc.preprocess([[orc.scene_load(v) for v in lod] for lod in verts])
    ow = wo.WangTile(pp)
    ou = ow.configure(wo.UserData(**FS.CFG))
    newest = FS.newest_events(plan["sched"])
    fcams = FS.frame_cams(plan["sched"])
    out, osd = {}, None
    with np.errstate(all="ignore"):
        for j, cam in enumerate(plan["cams"][:max(ANCHORS) + 1]):
            ecam = orc.Camera(FS.W, FS.HH, cam[0], cam[1], [0, 0, 1])
            if ow.check_update(cam[0]):
                osd = ow.build_tiles(cam[0])
            osort = ow.sort_tiles(cam[0], ecam.view_proj())
            if j not in ANCHORS:
                continue
            k = newest.index(j)
            fcam = orc.Camera(FS.W, FS.HH, fcams[k][0], fcams[k][1], [0, 0, 1])
            odraws = wo.renderer_draws(pp, osort, fcam.view_proj())      # the draw loop culls per frame, with the frame's camera
            out[(k, j)] = orc.render(fcam.uniforms(), wo.scene_uniforms_from_data(ou, osd["center_coord"]), pp.tex, odraws, FS.W, FS.HH)
    return out


@pytest.mark.parametrize("source", FS.SOURCES)
def test_replay_is_anchored_to_the_oracle(renderer, plan, oracle_frames, source):
    rep = _replay(renderer, plan, source)
    assert len(oracle_frames) == 3
    for (k, j), (ref, st) in oracle_frames.items():
        n_visible, n_pairs = rep.stats[(k, j)]
        err = H.max_abs_diff(rep[(k, j)], ref)
        print(f"{source}: frame {k} on event {j}: visible {n_visible} pairs {n_pairs} max |replay - oracle| {err:.3e}")
        assert n_visible == st["n_visible"] and n_pairs == st["n_pairs16"], (k, j)
        assert st["n_visible"] > 500
        assert err <= TOL, (k, j, err)
    renderer.synchronize()


def test_worker_thread_beside_the_render_thread(renderer):
    """The benchmark's arrangement: the device worker's calls come from a second host thread (check_update / build_tiles on the host,
    build_tiles / sort_tiles / fetch on the device worker), the render thread swaps the newest published event in and keeps every
    slot in flight, under DEFER_SWAP = 1 with the graph on.  No Python lock is held around a C call; `done` and `submitted` are plain
    integers each written by one thread."""
    import torch
    K, PACE, MAX_FRAMES, MAX_SECONDS = 24, 3, 400, 60.0
    slots = renderer.frame_slots()
    cams = [FS.PLACES[j % 3] if j % 2 else FS.crossing(0.25 * j) for j in range(K + 1)]      # event 0 first, then the K ordered cameras
    state = dict(done=1, submitted=0, stop=False, error=None)
    sus = []

    with renderer.options(TIMING=0, GRAPH=1, DEFER_SWAP=1, PAIR_CAP=0, NO_MERGE_REUSE=0):
        src = FS.EventSource(renderer, "worker")
        frames, images, windows, swaps, tickets, th = [], [], [], [(0, 0)], [], None
        try:
            sus.append(src.set(cams[0]))                     # the first event, synchronously
            wang, dev = src.wang, src.dev

            def work():
                try:
                    for j in range(1, K + 1):
                        while state["submitted"] < PACE * j:            # event j starts once 3 j frames have been submitted
                            if state["stop"]:
                                return
                            time.sleep(1e-4)
                        cam = cams[j]
                        src.build(cam)
                        dev.sort_tiles(cam[0], FS.camera(cam)[1])
                        dev.fetch()                          # publishes the event ...
                        sus.append(wang.scene_uniforms())
                        state["done"] += 1                   # ... before it is counted
                except BaseException as e:                   # noqa: BLE001 - reported by the render thread
                    state["error"] = e

            bufs = [torch.zeros((FS.HH, FS.W, 4), dtype=torch.float32, device="cuda") for _ in range(slots + 1)]
            torch.cuda.synchronize()
            th = threading.Thread(target=work, daemon=True)
            t_end = time.monotonic() + MAX_SECONDS
            th.start()
            swapped_at, b, tail = 1, 1, None
            stopped = None
            while True:
                if state["error"] is not None:
                    stopped = f"worker thread raised {state['error']!r}"
                elif len(frames) >= MAX_FRAMES:
                    stopped = f"{MAX_FRAMES} frames without the worker finishing (done = {state['done']})"
                elif time.monotonic() > t_end:
                    stopped = f"{MAX_SECONDS} s without the worker finishing (done = {state['done']}, {len(frames)} frames)"
                if stopped:
                    break
                a = state["done"]
                if a > swapped_at:
                    dev.swap_in(fetch=False)
                    b = state["done"]
                    swaps.append((a - 1, min(b, K)))         # the event taken: published before `a` was counted, at most the one being counted
                    swapped_at = a
                k = len(frames)
                if len(tickets) == slots:
                    t, q = tickets.pop(0)
                    renderer.render_wait(t)
                    images[q] = bufs[q % (slots + 1)].cpu().numpy()
                cam = FS._look(cams[min(b - 1, K)], k % 3)
                cu, _ = FS.camera(cam)
                su = sus[b - 1]
                images.append(None)
                tickets.append((renderer.render_async(cu, su, FS.W, FS.HH, bufs[k % (slots + 1)].data_ptr(), transmittance_eps=FS.T_EPS), k))
                frames.append((cu, su, b - 1))
                # this frame may read the list of the swap before the last one (still building: deferred) up to the last one's newest
                windows.append(list(range(swaps[-2][0] if len(swaps) > 1 else 0, swaps[-1][1] + 1)))
                state["submitted"] = len(frames)
                if tail is None and state["done"] == K + 1 and swapped_at == K + 1:
                    tail = slots                             # the worker has finished and its last event is in: `slots` more frames
                elif tail is not None:
                    tail -= 1
                    if tail <= 0:
                        break
            state["stop"] = True
            th.join(timeout=60)
            assert not th.is_alive(), "the worker thread did not end"
            assert stopped is None, stopped
            while tickets:
                t, q = tickets.pop(0)
                renderer.render_wait(t)
                images[q] = bufs[q % (slots + 1)].cpu().numpy()
            renderer.synchronize()
            # one more frame after synchronize(): nothing is pending any more, it reads what the last swap took
            cu, _ = FS.camera(FS._look(cams[K], 1))
            images.append(renderer.render(cu, sus[K], FS.W, FS.HH, transmittance_eps=FS.T_EPS))
            frames.append((cu, sus[K], K))
            windows.append(list(range(swaps[-1][0], swaps[-1][1] + 1)))
        finally:
            state["stop"] = True
            for t, _ in tickets:                             # (a failure above: no ticket stays behind on the session's renderer)
                renderer.render_wait(t)
            renderer.synchronize()
            if th is not None:
                th.join(timeout=60)
            if th is None or not th.is_alive():              # (never under a thread that may still call into the worker)
                src.close()
    rep = FS.replay(renderer, "worker", FS.needed_frames(frames, windows), cams=cams)
    matched = FS.match_stream(images, windows, rep)
    assert matched == sorted(matched)
    print(f"thread: {len(frames)} frames checked, {len(swaps) - 1} swap-ins, {len(set(matched))} distinct events read, "
          f"widest window {max(len(w) for w in windows)} events")
    assert len(swaps) - 1 >= K // 2
    assert len(set(matched)) >= 6
    renderer.synchronize()
