"""Python model of group8_select_kth32_top (hgx_device.h), control flow included: eight events side by
side in one wave, 8 lanes per event, one instruction stream.

Per event the arithmetic is wave_select_kth32_top's (ctsselref.select_top): values rebased to the event's
minimum, 6-bit digits from the top of the event's range (the last digit takes what is left), the exit as
soon as the chosen bin holds one value or at shift 0. What the group adds is modelled as the kernel does
it:
  - every event has its own lo, top, shift, rank, prefix and live flag; the pass loops are common, bounded
    at six passes in all, and end when no event of the group is live;
  - an event that takes no part (no member: absent, or a 64-bit event) and an event that has finished run
    along: their lanes add 0 to their own bins and their results stay what they were;
  - a value that no longer counts (not a member, or outside the chosen bin) adds 0 to the bin of its digit;
  - lane l of an event owns bins l + 8t: the chosen bin is found by walking the 8 row totals (the last row
    whose exclusive prefix is <= rank), then by an exclusive scan over the 8 lanes of that row;
  - the winner of a bin of one is the minimum over the values that still count;
  - after the first pass, when every live event of the group has at most CAP = 32 values left, each event's
    values are gathered into a list in lane order and the later passes run over CAP / 8 values per lane;
    otherwise all passes run over the vpl values per lane.

select_group(events) takes up to eight (values, member) pairs, member a boolean array over the values
(None: all), and returns (results, trail): results[i] is None for an event without members;
trail["passes"][i] counts the passes event i was live in, trail["exit"][i] names its way out as
ctsselref does, trail["loops"] is the common loop count and trail["listed"] says whether the later
passes ran over the lists.

form_groups(pos) gives the kernel's grouping of the positions of one chain: tiles of 64 positions, event
e = position % 64 of a tile belongs to group e % 8 (8 waves: wave e % 8; 4 waves: wave e % 4, its group
(e % 8) // 4) and is its slot e // 8.
"""
import numpy as np

DIGIT = 6
M32 = 0xFFFFFFFF
TILE = 64
CAP = 32


def max_passes():
    return (32 + DIGIT - 1) // DIGIT


class _Event:
    """One event's 8 lanes: d[l][q] = value q of lane l minus lo, act[l][q] = it still counts."""

    def __init__(self, vals, member, vpl):
        nv = vpl * 8
        v = np.asarray(vals, dtype=np.int64)
        assert v.size <= nv and (v.size == 0 or (int(v.min()) >= 0 and int(v.max()) <= M32))
        mem = np.ones(v.size, bool) if member is None else np.asarray(member, bool)
        # value c of the event (chain c) sits in lane c % 8, slot c // 8
        self.d = np.zeros(nv, np.int64)
        self.act = np.zeros(nv, bool)
        self.part = bool(mem.any())
        self.res, self.exit, self.passes = None, None, 0
        self.live, self.top, self.k, self.prefix, self.lo, self.cnt = False, 0, 0, 0, M32, 0
        if not self.part:
            return
        self.lo, hi = int(v[mem].min()), int(v[mem].max())
        self.d[:v.size] = (v - self.lo) & M32
        self.k = int(mem.sum()) // 2
        self.res = self.lo
        self.live = hi > self.lo
        self.top = (hi - self.lo).bit_length() if self.live else 0
        if self.live:
            self.act[:v.size] = mem
        else:
            self.exit = "range0"

    def lanes(self):
        """(d, act) as [lane][slot]."""
        return self.d.reshape(-1, 8).T, self.act.reshape(-1, 8).T

    def run_pass(self):
        shift = self.top - DIGIT if self.top > DIGIT else 0
        width = self.top - shift
        dig = (self.d >> shift) & ((1 << width) - 1)
        hist = np.bincount(dig, weights=self.act, minlength=64).astype(np.int64)
        if not self.live:
            assert not self.act.any()
            return
        assert 0 <= self.k < int(hist.sum())
        self.passes += 1
        h = hist.reshape(8, 8)            # h[t][l]: bin 8t + l, lane l
        acc = below = tsel = 0
        for t in range(8):
            if self.k >= acc:
                below, tsel = acc, t
            acc += int(h[t].sum())
        k1 = self.k - below
        incl = np.cumsum(h[tsel])
        excl = incl - h[tsel]
        own = np.nonzero((k1 >= excl) & (k1 < incl))[0]
        assert own.size == 1
        l = int(own[0])
        bucket, self.cnt = tsel * 8 + l, int(h[tsel][l])
        self.k = k1 - int(excl[l])
        self.prefix |= bucket << shift
        last, one = shift == 0, self.cnt == 1
        if not last:
            self.act &= dig == bucket
            assert int(self.act.sum()) == self.cnt
            if one:
                self.res = self.lo + int(np.where(self.act, self.d, M32).min())
                self.exit = "one"
        else:
            self.res = self.lo + self.prefix
            self.exit = "shift0"
        self.live = not last and not one
        if not self.live:
            self.act[:] = False
        self.top = shift

    def to_list(self):
        """The values that still count, lane by lane, as the event's new CAP values (CAP / 8 per lane)."""
        d, act = self.lanes()
        lst = np.concatenate([d[l][act[l]] for l in range(8)]) if self.live else np.zeros(0, np.int64)
        assert lst.size == (self.cnt if self.live else 0) and lst.size <= CAP
        self.d = np.zeros(CAP, np.int64)
        self.act = np.zeros(CAP, bool)
        self.d[:lst.size] = lst
        self.act[:lst.size] = True


def select_group(events, vpl=32):
    assert 1 <= len(events) <= 8
    ev = [_Event(v, m, vpl) for v, m in events]
    loops, listed = 0, False
    if any(e.live for e in ev):
        loops = 1
        for e in ev:
            e.run_pass()
        if any(e.live for e in ev):
            listed = vpl > CAP // 8 and not any(e.live and e.cnt > CAP for e in ev)
            if listed:
                for e in ev:
                    e.to_list()
            for _ in range(1, max_passes()):
                loops += 1
                for e in ev:
                    e.run_pass()
                if not any(e.live for e in ev):
                    break
    assert not any(e.live for e in ev), "select_group: the digits cover 32 bits"
    trail = {"passes": [e.passes for e in ev], "exit": [e.exit for e in ev], "loops": loops, "listed": listed}
    return [e.res for e in ev], trail


def form_groups(pos):
    """(tile, group, slot) of chain positions, counted from the first tile's start."""
    pos = np.asarray(pos)
    e = pos % TILE
    return pos // TILE, e % 8, e // 8
