"""KeyFrameDatabase — host-side mirror of ORB_SLAM2::KeyFrameDatabase over liborbx.

The keyframes' BowVectors live on the GPU (orbx_kfdb.hip); a query counts the
shared words of every entry and scores those above 0.8 of the maximum in two
kernels, and the covisibility accumulation runs on the host as in the reference:

    db = KeyFrameDatabase(voc, 4096, 2048, connected=..., covisibles=...)
    db.add(pKF)                                         # LocalMapping / LoopClosing
    cands = db.DetectLoopCandidates(pKF, minScore)      # LoopClosing::DetectLoop
    cands = db.DetectRelocalizationCandidates(F)        # Tracking::Relocalization
    scores = db.score_covisibles(pKF, kfs)              # the minScore loop of DetectLoop

`connected(kf)` and `covisibles(kf, n)` stand for KeyFrame::GetConnectedKeyFrames
and GetBestCovisibilityKeyFrames: callables that return keyframe objects (the
library has no covisibility graph). There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import ORBDB_LOOP, ORBDB_RELOC, OrbxError, ORBX_EINVAL, check, lib, ptr
from .vocabulary import bow_arrays


class KeyFrameDatabase:
    def __init__(self, voc_or_scoring, max_keyframes: int, word_pitch: int, *, device: int = 0, connected=None,
                 covisibles=None):
        scoring = voc_or_scoring if isinstance(voc_or_scoring, (int, np.integer)) else voc_or_scoring._info()[2]
        self.max_keyframes, self.word_pitch = int(max_keyframes), int(word_pitch)
        self.connected = connected or (lambda kf: ())
        self.covisibles = covisibles or (lambda kf, n: ())
        self._h = C.c_void_p(0)
        self._kfs = {}  # slot -> keyframe object
        check(lib().orbdb_create(device, self.max_keyframes, self.word_pitch, int(scoring), C.byref(self._h)),
              database=True)

    def close(self):
        if self._h and self._h.value:
            lib().orbdb_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def size(self) -> tuple:
        """(live entries, one past the highest slot in use)."""
        a, b = C.c_int(0), C.c_int(0)
        check(lib().orbdb_size(self._h, C.byref(a), C.byref(b)), database=True)
        return a.value, b.value

    # ---------------------------------------------------------- add / erase / clear
    def add(self, pKF) -> int:
        """KeyFrameDatabase::add (src/KeyFrameDatabase.cc:76-82); the slot is kept on pKF.mnDbSlot."""
        w, v = bow_arrays(pKF.mBowVec)
        slot = C.c_int(-1)
        check(lib().orbdb_add(self._h, ptr(w), ptr(v), len(w), C.byref(slot)), database=True)
        pKF.mnDbSlot = slot.value
        self._kfs[slot.value] = pKF
        return slot.value

    def erase(self, pKF) -> None:
        """KeyFrameDatabase::erase (:84-103)."""
        slot = self._slot(pKF)
        if slot < 0:
            raise OrbxError(ORBX_EINVAL, "keyframe is not in the database")
        check(lib().orbdb_erase(self._h, slot), database=True)
        del self._kfs[slot]
        pKF.mnDbSlot = -1

    def clear(self) -> None:
        """KeyFrameDatabase::clear (:105-109)."""
        check(lib().orbdb_clear(self._h), database=True)
        for kf in self._kfs.values():
            kf.mnDbSlot = -1
        self._kfs = {}

    def _slot(self, kf) -> int:
        s = getattr(kf, "mnDbSlot", -1)
        return s if s >= 0 and self._kfs.get(s) is kf else -1

    # ---------------------------------------------------------- queries
    def _detect(self, mode: int, q, exclude, min_score: float) -> list:
        w, v = bow_arrays(q.mBowVec)
        ex = np.array(sorted({s for s in (self._slot(k) for k in exclude) if s >= 0}), np.int32)
        cap = max(self.size()[1], 1)
        slots, scores = np.zeros(cap, np.int32), np.zeros(cap, np.float32)
        n, minc = C.c_int(0), C.c_int(0)
        check(lib().orbdb_query(self._h, mode, ptr(w), ptr(v), len(w), ptr(ex) if len(ex) else None, len(ex),
                                C.c_float(min_score), ptr(slots), ptr(scores), cap, C.byref(n), C.byref(minc)),
              database=True)
        self.last_list = [(float(scores[i]), self._kfs[int(slots[i])]) for i in range(n.value)]  # lScoreAndMatch
        self.last_min_common = minc.value
        if n.value == 0:
            return []
        neigh = np.full((n.value, 10), -1, np.int32)
        for i in range(n.value):
            for k, kf in enumerate(list(self.covisibles(self._kfs[int(slots[i])], 10))[:10]):
                neigh[i, k] = self._slot(kf)
        out, nout = np.zeros(n.value, np.int32), C.c_int(0)
        check(lib().orbdb_select_candidates(self._h, mode, ptr(slots), ptr(scores), n.value, ptr(neigh),
                                            C.c_float(min_score), ptr(out), C.byref(nout)), database=True)
        return [self._kfs[int(s)] for s in out[:nout.value]]

    def DetectLoopCandidates(self, pKF, minScore: float) -> list:
        """KeyFrameDatabase::DetectLoopCandidates (:112-233)."""
        return self._detect(ORBDB_LOOP, pKF, self.connected(pKF), float(minScore))

    def DetectRelocalizationCandidates(self, F) -> list:
        """KeyFrameDatabase::DetectRelocalizationCandidates (:235-345)."""
        return self._detect(ORBDB_RELOC, F, (), 0.0)

    def score_covisibles(self, pKF, kfs) -> np.ndarray:
        """mpORBVocabulary->score(pKF->mBowVec, kf->mBowVec) for keyframes of the database
        (LoopClosing::DetectLoop, src/LoopClosing.cc:147-165), as float64."""
        w, v = bow_arrays(pKF.mBowVec)
        kfs = list(kfs)
        slots = np.array([self._slot(k) for k in kfs], np.int32)
        out = np.zeros(len(kfs), np.float64)
        check(lib().orbdb_score_slots(self._h, ptr(w), ptr(v), len(w), ptr(slots), len(slots), ptr(out)),
              database=True)
        return out
