"""Key-point tracks: a table of slots that follows points over the frames of a video and gives each a persistent id.

`frames.FrameSequence(model, keypoints=det, tracks=True)` keeps one `TrackTable` and runs three operations on it per pair
(csrc/tracks.hip; the definitions are in include/focusflow_hip.h):

    ops.tracks_replenish    the detector's points of the first frame fill the free slots, unless a live track is nearer than
                            the detector's min_distance; every birth takes the next id
    ops.tracks_mask         the live positions as the 0 / 255 mask FF-RAFT reads for the first frame
    ops.tracks_advance      every live track moves by the flow sampled bilinearly at its sub-pixel position, ages, or dies
                            when its target leaves the frame

A dead slot holds ids = -1, pos = -1, age = 0.  Ids are never reused: `next_id` only counts up, through reset() too.
"""
from typing import NamedTuple

import torch

MAX_SLOTS = 4096      # csrc/tracks.hip: one block keeps a sample's table in LDS


class TrackResult(NamedTuple):
    """What a pair adds to a FrameResult in tracks mode: per slot, the id and age the track had BEFORE this pair's advance
    (-1 and 0 for a slot that was dead), and per sample the number of tracks born in front of this pair."""
    ids: torch.Tensor
    age: torch.Tensor
    born: torch.Tensor


class TrackTable:
    """The state of `b` samples with `n` slots each: pos (b,n,2) fp32 [x, y] in coordinates of the unpadded frame, ids (b,n)
    int64, age (b,n) int32 (pairs survived), next_id (b) int64 (the id of the next birth)."""

    def __init__(self, b, n, device):
        if int(b) < 1:
            raise ValueError(f"b={b}: at least one sample")
        if not 1 <= int(n) <= MAX_SLOTS:
            raise ValueError(f"tracks: {n} slots, 1 .. {MAX_SLOTS} are possible")
        self.b, self.n = int(b), int(n)
        self.pos = torch.empty((self.b, self.n, 2), dtype=torch.float32, device=device)
        self.ids = torch.empty((self.b, self.n), dtype=torch.int64, device=device)
        self.age = torch.empty((self.b, self.n), dtype=torch.int32, device=device)
        self.next_id = torch.zeros((self.b,), dtype=torch.int64, device=device)
        self.reset()

    def _tensors(self):
        return self.pos, self.ids, self.age, self.next_id

    def reset(self):
        """Every slot dies.  next_id keeps counting, so ids stay unique over the whole session."""
        self.pos.fill_(-1.0)
        self.ids.fill_(-1)
        self.age.zero_()

    def state(self):
        """(pos, ids, age, next_id) as clones: what load_state() puts back."""
        return tuple(t.clone() for t in self._tensors())

    def load_state(self, state):
        for t, saved in zip(self._tensors(), state):
            t.copy_(saved)

    @property
    def live(self):
        """(b,n) bool: the slot holds a track."""
        return self.ids >= 0

    def __repr__(self):
        return f"TrackTable(b={self.b}, n={self.n}, device={self.pos.device})"
