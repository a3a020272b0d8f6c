"""CPU check of the taps' host-side bookkeeping (sdr-j-fm_amd/csrc/fmx_taps.h): RecordTap -- the modulation, programme audio, reception and RDS meters --
and SlotTap -- the spectrum and multiplex spectrum meters, the sub-carrier decoder, the monitoring feed.  The header's own functions, compiled for the host
(tests/taps_check.cpp), against a brute-force model: per unit a dict from ring slot to the item it holds, cursors and switches as plain integers.  Seeded
random sequences of switch, flush, piece, setup, growth and read-out, with each tap's own ring size and with a ring of 4; then, per tap, the order of calls
of its stage function replayed on the header alone against values worked out by hand."""
import json
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdr-j-fm_amd", "csrc")


def ring_of(header):
    """`constexpr int RING = N;` of a tap's header (the reception meter's is the modulation meter's)."""
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"constexpr int RING = (\w+(?:::\w+)?);", text)
    return int(m.group(1)) if m.group(1).isdigit() else ring_of("fmx_%s.h" % m.group(1).split("::")[0])


RECORD_RINGS = {"mod": ring_of("fmx_meter.h"), "audio": ring_of("fmx_loud.h"), "rx": ring_of("fmx_rx.h"), "rdsm": ring_of("fmx_rdsm.h"), "small": 4}
SLOT_RINGS = {"spec": ring_of("fmx_spec.h"), "mpx": ring_of("fmx_mpx.h"), "sca": ring_of("fmx_sca.h"), "feed": ring_of("fmx_feed.h"), "small": 4}


@pytest.fixture(scope="module")
def taps(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("taps") / "taps_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "taps_check.cpp")])

    def run(queries):
        """One process, one RecordTap and one SlotTap: the queries in order."""
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [json.loads(line) for line in out]
    return run


class Script:
    """Queries with the check of each answer; the model runs while the script is written, the program when it is played."""

    def __init__(self):
        self.steps = []

    def ask(self, query, check=None):
        self.steps.append((query, check))

    def play(self, taps):
        for (query, check), got in zip(self.steps, taps([q for q, _ in self.steps])):
            assert "error" not in got, query
            if check is not None:
                check(got, query)


def expect(**want):
    want = {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in want.items()}      # (a copy: the model moves on)

    def check(got, query):
        for k, v in want.items():
            assert got[k] == v, (query, k, got[k], v)
    return check


# ---- the slot taps against the model
class SlotModel:
    def __init__(self, units, ring):
        self.units, self.ring = units, ring
        self.user = [0] * units
        self.started = False
        self.call = [0] * units
        self.slot = [-1] * units
        self.slots = 0
        self.on_from = [-1] * units
        self.cursor = [0] * units
        self.held = [dict() for _ in range(units)]      # ring slot -> item
        self.next_item = 0                               # (a piece's position is the index of its first item)

    def tags(self):
        return [self.held[u].get(k, -1) for u in range(self.units) for k in range(self.ring)]

    def unread(self, u):
        return sorted(i for i in self.held[u].values() if i >= self.cursor[u])


def slot_script(units, ring, seed, steps=400):
    rng = random.Random(seed)
    M, S = SlotModel(units, ring), Script()
    S.ask("s_init %d" % units, expect(user=[0] * units, slot=[], slots=0, cap=0, live=0))

    def state():
        if not M.started:
            return expect(user=M.user, slot=[], tags=[])
        return expect(user=M.user, call=M.call, slot=M.slot, on_from=M.on_from, cursor=M.cursor, tags=M.tags(), slots=M.slots)

    def flush():      # (flush_mailbox: memory for the units switched on, then the piece's values)
        if any(M.user):
            S.ask("s_start %d %d" % (units, ring))
            M.started = True
            new = [u for u in range(units) if M.user[u] and M.slot[u] < 0]      # (only units that are on and have no slot)
            S.ask("s_needed", expect(needed=len(new)))
            for u in new:                                                       # (dense, in switch-on order; a unit keeps its slot)
                M.slot[u] = M.slots
                M.slots += 1
            S.ask("s_grow", expect(slot=M.slot, slots=M.slots, cap=M.slots))
            assert sorted(s for s in M.slot if s >= 0) == list(range(M.slots))
        if M.started:
            M.call = list(M.user)
        S.ask("s_switches", state())

    def piece():
        pos = M.next_item
        k = rng.choice([0, 1, 1, 2, 3, ring - 1, ring, ring + 3])
        for u in range(units):
            if not M.call[u]:
                M.on_from[u] = -1                      # (off in any piece: -1 and no job)
            elif M.on_from[u] < 0:
                M.on_from[u] = pos                     # (the first piece on: its start; staying on changes nothing)
            S.ask("s_begin %d %d" % (u, pos), expect(job=1 if M.call[u] else 0, on_from=M.on_from))
        for u in range(units):
            if not M.call[u]:
                continue
            for item in range(max(pos, pos + k - ring), pos + k):      # (of a long piece only the last `ring` items are formed)
                if item >= M.on_from[u] and rng.random() > 0.15:       # (an item may not be delivered: a gap)
                    M.held[u][item % ring] = item
                    S.ask("s_tag %d %d" % (u, item))
        M.next_item = pos + k
        S.ask("s_live 1", state())

    def read_run():
        u, cap = rng.randrange(units), rng.choice([1, 2, 3, ring, ring + 5])
        have = set(M.unread(u))
        first, n = (min(have), 0) if have else (-1, 0)
        while have and n < cap and first + n in have:      # (ends at the first gap or at the capacity)
            n += 1
        assert n <= ring
        S.ask("s_run %d %d" % (u, cap), expect(**{"from": first, "count": n}))
        if n:
            M.cursor[u] = first + n
            S.ask("s_commit %d %d" % (u, M.cursor[u]), state())

    for _ in range(steps):
        op = rng.random()
        if not M.started or op < 0.2:
            u = rng.randrange(units)
            M.user[u] = rng.choice([0, 0, 1, 67000, 3]) if M.user[u] else rng.choice([1, 92000, 2])
            S.ask("s_user %d %d" % (u, M.user[u]))
            flush()
        elif op < 0.55:
            flush()
            piece()
        elif op < 0.70:
            u = rng.randrange(units)
            want = M.unread(u)
            cap = rng.choice([1, 2, ring, ring + 5])
            S.ask("s_pending %d %d" % (u, cap), expect(items=want[:cap]))
            if want[:cap]:
                M.cursor[u] = want[:cap][-1] + 1
                S.ask("s_commit %d %d" % (u, M.cursor[u]), state())
                S.ask("s_pending %d %d" % (u, 2 * ring), expect(items=want[cap:]))      # (nothing at or below the last item handed out comes again)
        elif op < 0.85:
            read_run()
        elif op < 0.92:
            u = rng.randrange(units)      # (another centre, another mode: as off followed by on -- the next piece on starts at its own start)
            M.on_from[u] = -1
            S.ask("s_restart_unit %d" % u, state())
            if M.call[u]:
                M.on_from[u] = M.next_item
                S.ask("s_begin %d %d" % (u, M.next_item), expect(job=1, on_from=M.on_from))
        else:
            # a setup taken over: no tagged item is left, every cursor is 0, the slots are kept; the indices start over
            M.on_from = [-1] * units
            M.cursor = [0] * units
            M.held = [dict() for _ in range(units)]
            M.next_item = 0
            S.ask("s_restart", expect(slot=M.slot, slots=M.slots, tags=[-1] * (units * ring), cursor=[0] * units, on_from=[-1] * units))
    return S


@pytest.mark.parametrize("name", sorted(SLOT_RINGS))
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_slot_tap_against_model(taps, name, seed):
    """Switching, slots, pieces, setups and both kinds of read-out in random order: after every step the header's state is the model's."""
    slot_script(units=5, ring=SLOT_RINGS[name], seed=seed * 101 + SLOT_RINGS[name]).play(taps)


def test_slot_tap_overwritten_items_are_absent(taps):
    """A reader that never reads: the ring holds the newest items only, `pending` hands out those and `run` starts at the oldest of them."""
    S = Script()
    for q in ("s_init 2", "s_user 1 1", "s_start 2 4", "s_grow", "s_switches", "s_begin 1 0"):
        S.ask(q)
    for item in range(11):
        S.ask("s_tag 1 %d" % item)
    S.ask("s_pending 1 64", expect(items=[7, 8, 9, 10]))
    S.ask("s_pending 1 3", expect(items=[7, 8, 9]))
    S.ask("s_run 1 64", expect(**{"from": 7, "count": 4}))
    S.ask("s_commit 1 9")
    S.ask("s_tag 1 12")                                    # (11 was not delivered: slot 3 still holds 7, which is behind the cursor)
    S.ask("s_pending 1 64", expect(items=[9, 10, 12]))
    S.ask("s_run 1 64", expect(**{"from": 9, "count": 2}))
    S.ask("s_pending 0 64", expect(items=[]))
    S.ask("s_run 0 64", expect(**{"from": -1, "count": 0}))
    S.play(taps)


def test_slot_tap_slots_across_off_and_on(taps):
    """Slots are dense and in switch-on order, a unit keeps its slot across off and on, and slots_needed counts only units that are on without one."""
    S = Script()
    S.ask("s_init 4", expect(slot=[]))
    S.ask("s_user 2 1")
    S.ask("s_start 4 4", expect(slot=[-1, -1, -1, -1], on_from=[-1] * 4, cursor=[0] * 4, call=[0] * 4, tags=[-1] * 16))
    S.ask("s_needed", expect(needed=1))
    S.ask("s_grow", expect(slot=[-1, -1, 0, -1], slots=1, cap=1))
    S.ask("s_user 2 0")
    S.ask("s_user 0 1")
    S.ask("s_needed", expect(needed=1))
    S.ask("s_grow", expect(slot=[1, -1, 0, -1], slots=2, cap=2))
    S.ask("s_user 2 1")                                    # (on again: its slot is still 0)
    S.ask("s_user 3 1")
    S.ask("s_user 1 1")
    S.ask("s_needed", expect(needed=2))
    S.ask("s_start 4 4", expect(slot=[1, -1, 0, -1]))      # (a later start changes nothing)
    S.ask("s_grow", expect(slot=[1, 2, 0, 3], slots=4, cap=4))
    S.ask("s_needed", expect(needed=0))
    S.ask("s_restart", expect(slot=[1, 2, 0, 3], slots=4, cap=4))
    S.play(taps)


# ---- the record taps against the model
def record_script(channels, ring, seed, steps=400):
    rng = random.Random(seed)
    S = Script()
    user, call, on_from, produced, cursor = [0] * channels, [0] * channels, [-1] * channels, [0] * channels, [0] * channels
    alloc, pos = False, 0
    S.ask("r_init %d" % channels, expect(user=user, cursor=cursor, call=[], alloc=0))
    for _ in range(steps):
        op = rng.random()
        if op < 0.2:
            c = rng.randrange(channels)
            user[c] ^= 1
            S.ask("r_user %d %d" % (c, user[c]), expect(user=user))
        elif op < 0.6:
            if not alloc and any(user):                    # (the first piece in which a meter is on: the device side, and the books start)
                alloc = True
                S.ask("r_start %d" % channels, expect(call=[0] * channels, on_from=[-1] * channels, produced=[0] * channels, cursor=[0] * channels, alloc=1))
            if alloc:
                call = list(user)
            S.ask("r_switches", expect(call=call if alloc else [], alloc=int(alloc)))
            if not alloc:
                continue
            n = rng.choice([1, 50, 500])
            for c in range(channels):
                if not call[c]:
                    on_from[c] = -1
                elif on_from[c] < 0:
                    on_from[c] = pos
                S.ask("r_begin %d %d" % (c, pos), expect(job=call[c], on_from=on_from))
                if call[c]:
                    produced[c] += rng.choice([0, 0, 1, 2, ring - 1, ring, 3 * ring + 1])
                    S.ask("r_produced %d %d" % (c, produced[c]), expect(produced=produced))
            pos += n
        elif alloc:
            c, cap = rng.randrange(channels), rng.choice([0, 1, 3, ring, ring + 9])
            have = list(range(max(cursor[c], produced[c] - ring), produced[c]))[:cap]      # (a reader more than a ring behind has lost the oldest)
            frm = have[0] if have else max(cursor[c], produced[c] - ring)
            want = [frm, len(have), frm + len(have)]
            commit = rng.random() < 0.7
            if commit:
                cursor[c] = want[2]
            S.ask("%s %d %d %d" % ("r_read" if commit else "r_take", c, ring, cap),
                  expect(**{"from": want[0], "count": want[1], "next": want[2], "want": want, "cursor": cursor}))
    return S


@pytest.mark.parametrize("name", sorted(RECORD_RINGS))
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_record_tap_against_model(taps, name, seed):
    """Switching, pieces and read-outs in random order: the on/off rule, and take / commit equal to ring_take on the same integers."""
    record_script(channels=4, ring=RECORD_RINGS[name], seed=seed * 77 + RECORD_RINGS[name]).play(taps)


# ---- each tap's stage function, replayed
def replay(taps, head, pieces):
    """pieces: (queries, on_from, produced | None) -- the trail behind each piece, worked out by hand."""
    S = Script()
    for q in head:
        S.ask(q)
    for queries, on_from, produced in pieces:
        for q in queries[:-1]:
            S.ask(q)
        S.ask(queries[-1], expect(on_from=on_from) if produced is None else expect(on_from=on_from, produced=produced))
    S.play(taps)


def test_stage_meter_order(taps):
    """stage_meter: windows of 9600 fm samples.  A piece whose first whole window begins at or behind its end pushes no job and leaves `produced` alone."""
    replay(taps, ["r_init 1", "r_user 0 1", "r_start 1", "r_switches"], [
        (["r_begin 0 1000"], [1000], [0]),                                # [1000, 5000): the first boundary is 9600 >= 5000 -- no job, nothing stored
        (["r_begin 0 5000"], [1000], [0]),                                # [5000, 9000): still in front of 9600
        (["r_begin 0 9000", "r_produced 0 2"], [1000], [2]),              # [9000, 30000): from 9600, windows 1 and 2 end in it
        (["r_user 0 0", "r_switches", "r_begin 0 30000"], [-1], [2]),     # off: no job, the window in progress dropped, the count stays
        (["r_user 0 1", "r_switches", "r_begin 0 38400", "r_produced 0 3"], [38400], [3]),      # [38400, 48000): on at a boundary, window 4 ends in it
    ])


def test_stage_rx_order(taps):
    """stage_rx: the same rule on the same grid; a job that completes no window stores the count it found."""
    replay(taps, ["r_init 2", "r_user 1 1", "r_start 2", "r_switches"], [
        (["r_begin 0 0", "r_begin 1 0", "r_produced 1 1"], [-1, 0], [0, 1]),                    # [0, 9600): channel 1 on at 0, window 0 ends in it
        (["r_begin 0 9600", "r_begin 1 9600", "r_produced 1 1"], [-1, 0], [0, 1]),              # [9600, 12000): a job, no window
        (["r_user 1 0", "r_switches", "r_begin 0 12000", "r_begin 1 12000"], [-1, -1], [0, 1]),
        (["r_user 1 1", "r_switches", "r_begin 0 12001", "r_begin 1 12001"], [-1, 12001], [0, 1]),      # [12001, 19000): the boundary 19200 is behind it -- no job
    ])


def test_stage_audio_meter_order(taps):
    """stage_audio_meter: windows of 4800 frames; every metered channel gets a job in every piece (the filters run), so `produced` is stored every time."""
    replay(taps, ["r_init 1", "r_user 0 1", "r_start 1", "r_switches"], [
        (["r_begin 0 100", "r_produced 0 0"], [100], [0]),                # [100, 1100): a job (reset), no window
        (["r_begin 0 1100", "r_produced 0 1"], [100], [1]),               # [1100, 10100): from 4800, window 1 ends in it
        (["r_user 0 0", "r_switches", "r_begin 0 10100"], [-1], [1]),
        (["r_user 0 1", "r_switches", "r_begin 0 10200", "r_produced 0 1"], [10200], [1]),
    ])


def test_stage_rds_meter_order(taps):
    """stage_rds_meter: on_from is what rdsm::piece returns -- no begin --, windows of 2560 RDS samples of the channel's own count."""
    replay(taps, ["r_init 1", "r_user 0 1", "r_start 1", "r_switches"], [
        (["r_on_from 0 -1"], [-1], [0]),                                  # the decoder is off: the piece changes nothing
        (["r_on_from 0 0", "r_produced 0 1"], [0], [1]),                  # samples [0, 3000): on at 0, window 0 ends in it
        (["r_user 0 0", "r_switches", "r_on_from 0 0"], [0], [1]),        # meter off, no samples (m1 = m0): nothing changes, a window may span the piece
        (["r_on_from 0 -1"], [-1], [1]),                                  # meter off with samples: the window in progress is dropped
    ])


def slot_head(units, ring, unit, value):
    return ["s_init %d" % units, "s_user %d %d" % (unit, value), "s_start %d %d" % (units, ring), "s_grow", "s_switches"]


def test_stage_spectrum_and_mpx_order(taps):
    """stage_spectrum / stage_mpx: begin per unit, then the tags of the records the piece delivers (here B = 2 blocks per record: record r needs its first block
    2 r at or behind the unit's first block)."""
    for ring in (SLOT_RINGS["spec"], SLOT_RINGS["mpx"]):
        replay(taps, slot_head(2, ring, 1, 1), [
            (["s_begin 0 0", "s_begin 1 0", "s_tag 1 0", "s_tag 1 1"], [-1, 0], None),                       # blocks 0 .. 3: records 0 and 1
            (["s_begin 0 16384", "s_begin 1 16384", "s_tag 1 2"], [-1, 0], None),                            # staying on
            (["s_user 1 0", "s_switches", "s_begin 0 24576", "s_begin 1 24576"], [-1, -1], None),            # off: no job, no tag
            (["s_user 1 1", "s_switches", "s_begin 0 28672", "s_begin 1 28672", "s_tag 1 4"], [-1, 28672], None),      # on in block 7: record 3 (blocks 6, 7) is not delivered
        ])
        got = taps(slot_head(2, ring, 1, 1) + ["s_begin 1 0", "s_tag 1 0", "s_tag 1 1", "s_tag 1 2", "s_tag 1 4", "s_pending 1 8"])[-1]
        assert ring == 4 and got["items"] == [1, 2, 4]      # (record 4 lies where record 0 lay)


def test_stage_sca_order(taps):
    """stage_sca: a centre other than the one the slot's taps were made for restarts the unit before begin."""
    ring = SLOT_RINGS["sca"]
    replay(taps, slot_head(1, ring, 0, 67000), [
        (["s_restart_unit 0", "s_begin 0 0", "s_tag 0 0"], [0], None),                                       # the first centre: taps, then on at 0
        (["s_begin 0 1920", "s_tag 0 1"], [0], None),
        (["s_user 0 92000", "s_switches", "s_restart_unit 0", "s_begin 0 3840", "s_tag 0 2"], [3840], None),      # another centre: as off followed by on
        (["s_user 0 0", "s_switches", "s_begin 0 5760"], [-1], None),
        (["s_user 0 92000", "s_switches", "s_begin 0 7680"], [7680], None),                                  # the same centre again: no restart, on at the piece's start
    ])


def test_stage_feed_order(taps):
    """stage_feed: another mode restarts the unit; a piece without a frame still takes the switches (begin runs, nothing is tagged)."""
    ring = SLOT_RINGS["feed"]
    replay(taps, slot_head(1, ring, 0, 1), [
        (["s_restart_unit 0", "s_begin 0 0"], [0], None),                                                    # frames <= 0: the bookkeeping only
        (["s_begin 0 0", "s_tag 0 0", "s_tag 0 1"], [0], None),
        (["s_user 0 2", "s_switches", "s_restart_unit 0", "s_begin 0 960", "s_tag 0 2"], [960], None),       # mode 1 -> 2
        (["s_user 0 0", "s_switches", "s_begin 0 1440"], [-1], None),
    ])
