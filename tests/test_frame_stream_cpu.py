"""The frame-stream harness without a GPU (tests/frame_stream.py): the window model against hand-written tables, and the promises
the scripted schedule makes, checked with host.WangTile alone."""
import functools

from tests import frame_stream as FS

E, F, S = ("event", None), ("frame", None), ("sync",)


def test_windows_without_deferral():
    #           e0 f  f  e1 f  e2 e3 f  S  f
    sched = [E, F, F, E, F, E, E, F, S, F]
    assert FS.allowed_events(sched, 0) == [[0], [0], [1], [3], [3]]
    assert FS.newest_events(sched) == [0, 0, 1, 3, 3]


def test_windows_with_a_deferred_swap_in():
    # the first event has nothing before it; a later one may still be building when a frame is submitted
    assert FS.allowed_events([E, F, F, E, F, F], 1) == [[0], [0], [0, 1], [0, 1]]
    # event on pending: e2 makes e1 current, whatever e1's build is doing; e0 can no longer be read
    assert FS.allowed_events([E, F, E, E, F, F], 1) == [[0], [1, 2], [1, 2]]
    # three in a row: only the last two remain
    assert FS.allowed_events([E, E, E, E, F], 1) == [[2, 3]]
    # synchronize() also waits for the build: the next frame reads the newest list -- until another event follows
    assert FS.allowed_events([E, F, E, F, S, F, F, E, F, S, F], 1) == [[0], [0, 1], [1], [1], [1, 2], [2]]
    # a synchronize() with nothing pending, and in front of the first event, changes nothing
    assert FS.allowed_events([S, E, S, F, E, F], 1) == [[0], [0, 1]]
    for sched in ([E, F, F, E, F, F], [E, F, E, E, F, F], [E, E, E, E, F]):
        for win, n in zip(FS.allowed_events(sched, 1), FS.newest_events(sched)):
            assert win[-1] == n and win[0] >= n - 1


def test_windows_with_a_fixed_frame_count():
    # value 3: two more frames on the old list, the third reads the new one; exact, no timing in it
    assert FS.allowed_events([E, F, E, F, F, F, F], 3) == [[0], [0], [0], [1], [1]]
    # the first event is current at once
    assert FS.allowed_events([E, F, F, F], 3) == [[0], [0], [0]]
    # event on pending: e2 makes e1 current at once and restarts the count
    assert FS.allowed_events([E, F, E, F, E, F, F, F], 3) == [[0], [0], [1], [1], [2]]
    # back to back: the first of the two is current for exactly two frames
    assert FS.allowed_events([E, E, E, F, F, F], 3) == [[1], [1], [2]]
    # synchronize() plays no part
    assert FS.allowed_events([E, F, E, S, F, S, F, F], 3) == [[0], [0], [0], [1]]
    # value 2: one more frame
    assert FS.allowed_events([E, F, E, F, F], 2) == [[0], [0], [1]]


@functools.lru_cache(maxsize=1)
def _events():
    return FS.host_events(FS.event_cams(FS.make_schedule()))


def test_schedule_has_the_promised_shapes():
    slots = FS.DEFAULT_SLOTS
    sched = FS.make_schedule(slots)
    kinds = [st[0] for st in sched]
    n_frames, n_events = kinds.count("frame"), kinds.count("event")
    assert 50 <= n_frames <= 70 and 25 <= n_events <= 40, (n_frames, n_events)
    assert kinds.count("sync") >= 1
    assert FS.burst_length(sched) == slots + 7
    text = "".join(k[0] for k in kinds)                      # e / f / s
    assert "efffefffefff" in text                            # events every third frame
    assert "fee" + "f" in text                               # two events with no frame between them
    assert "f" * slots + "e" in text                         # an event directly after `slots` frames nothing has collected
    burst = text.index("e" * (slots + 7))
    assert text[burst - 2 * slots:burst] == "ef" * slots     # the frames in flight at the burst: one per event, each on its own set
    assert text[burst + slots + 7] == "f"
    assert "sf" in text
    # the schedule scales with the slot count
    assert FS.burst_length(FS.make_schedule(3)) == 10


def test_schedule_rebuilds_and_changes_the_draw_list():
    ev = _events()
    assert ev[0][0]                                          # the first event builds the map
    moved = sum(1 for a, b in zip(ev, ev[1:]) if b[0] and b[1] != a[1])
    assert moved >= 2, [e[:2] for e in ev]                   # rebuilds that change center_coord
    differ = sum(1 for a, b in zip(ev, ev[1:]) if a[3] != b[3])
    assert differ >= 20, differ
    # the round-robin laps come back to the same members: the lists of a place's later visits are what the device copies
    cams = FS.event_cams(FS.make_schedule())
    laps = [j for j, c in enumerate(cams) if c in FS.PLACES][:9]
    assert laps == list(range(laps[0], laps[0] + 9))
    # a frame's scene uniforms follow the newest event
    frames = FS.schedule_frames(FS.make_schedule(), ev)
    assert len({bytes(su) for _, su, _ in frames}) >= 3


def test_every_window_of_the_schedule_is_small():
    sched = FS.make_schedule()
    n = FS.newest_events(sched)
    for defer in (0, 1, 3):
        wins = FS.allowed_events(sched, defer)
        assert len(wins) == len(n)
        for k, win in enumerate(wins):
            assert 1 <= len(win) <= 2 and win == sorted(win) and win[-1] <= n[k], (defer, k, win)
            if defer != 1:
                assert len(win) == 1
    # deferral shows in the schedule: some frames may read the previous list, some (value 3) must
    assert sum(len(w) == 2 for w in FS.allowed_events(sched, 1)) >= 20
    assert sum(w[0] < m for w, m in zip(FS.allowed_events(sched, 3), n)) >= 15
    assert FS.allowed_events(sched, 0) == [[m] for m in n]
