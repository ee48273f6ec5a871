"""Test infrastructure: a pure-Python model of the event-id index (babble_amd/csrc/hgx_idindex.h).

home slot = id bytes 0..7 little-endian & (slots - 1), tag = id bytes 8..11 little-endian, linear probing
by +1 with wrap-around, word = (tag << 32) | (gid + 1), slots = the smallest power of two >= 2 x capacity.
For linear probing the occupied slots, the summed displacement and the number of wrapped entries depend
on the key set alone, so this sequential model predicts what the device's concurrent inserts leave.
Nothing here is product code.
"""
from __future__ import annotations

import numpy as np


def slots_for(capacity: int) -> int:
    s = 2
    while s < 2 * capacity:
        s <<= 1
    return s


def home(id32, slots: int) -> int:
    return int.from_bytes(bytes(id32[:8]), "little") & (slots - 1)


def tag(id32) -> int:
    return int.from_bytes(bytes(id32[8:12]), "little")


class Model:
    def __init__(self, capacity: int):
        self.slots = slots_for(capacity)
        self.tab = [0] * self.slots
        self.rows = []

    def insert(self, id32) -> int:
        gid = len(self.rows)
        self.rows.append(bytes(id32))
        s = home(id32, self.slots)
        for _ in range(self.slots):
            if self.tab[s] == 0:
                self.tab[s] = (tag(id32) << 32) | (gid + 1)
                return gid
            s = (s + 1) & (self.slots - 1)
        raise AssertionError("table full")

    def find(self, id32) -> int:
        key, t, best = bytes(id32), tag(id32), -1
        s = home(id32, self.slots)
        for _ in range(self.slots):
            w = self.tab[s]
            if w == 0:
                return best
            g = (w & 0xFFFFFFFF) - 1
            if (w >> 32) == t and self.rows[g] == key and (best < 0 or g < best):
                best = g
            s = (s + 1) & (self.slots - 1)
        raise AssertionError("no empty slot")

    def state(self) -> dict:
        disp = wrapped = entries = 0
        for s, w in enumerate(self.tab):
            if w:
                h = home(self.rows[(w & 0xFFFFFFFF) - 1], self.slots)
                entries += 1
                disp += (s - h) & (self.slots - 1)
                wrapped += s < h
        return dict(kept=1, slots=self.slots, entries=entries, total_displacement=disp, wrapped=wrapped)


def model_of(ids, capacity: int) -> Model:
    m = Model(capacity)
    for r in np.asarray(ids, np.uint8).reshape(-1, 32):
        m.insert(r)
    return m


def forge_same_home_and_tag(id32) -> np.ndarray:
    """An id sharing bytes 0..11 with id32 (same home, same tag) whose row differs."""
    f = np.array(id32, np.uint8).copy()
    f[12:] ^= 0xA5
    return f


def forge_home(slot: int, salt: int = 0) -> np.ndarray:
    """An id whose home is `slot` in any table of more than `slot` slots (bytes 0..7 = slot)."""
    f = np.full(32, 0xC3 ^ (salt & 0xFF), np.uint8)
    f[:8] = np.frombuffer(int(slot).to_bytes(8, "little"), np.uint8)
    return f
