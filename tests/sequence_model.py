"""Random call sequences on shared slots, and a model of what include/wm.h says each call does to a slot.

generate(seed, n_ops) draws a sequence of API calls from a seeded rng: every step names a slot (0, 1, 2 or WM_SLOT_SYNC), a mask and
one of the engine's calls; output planes come from a small pool that all slots share, so slots overwrite each other's last output.
Model is a plain restatement of wm.h's slot rules -- what WM_MEM_SLOT_OUT names, whether a Gram hand-over is pending and of which
kind, which library writes end it, which detector takes it -- and predicts for every step the path the engine takes (ordinary,
promised, checked with its trusted / redone frames, fused), the launches of the four Gram kernels and the checked hand-over's
counters.  tests/test_gpu_sequences.py runs the sequences and holds the engine to an isolated replay and to these predictions;
tests/test_sequence_model.py checks generator and model on the CPU.  No GPU, no torch, no engine code in here.

The pool is POOL_FRAMES frames of one allocation; a plane is a run of frames (start, n).  Buffer b is the frames [3 b, 3 b + 3).
Slots are streams: two slots touching the same frames without a wm_sync between them is the CALLER's race (wm.h: "concurrency is by
slot"), so the generator syncs a slot before another slot writes what it still reads or writes, or reads what it still writes.
"""
import collections

import numpy as np

R, C = 40, 272              # the smallest plane with overlapped aligned strips and a hand-over instantiation
TILE = 32                   # 1 x 8 tiles
NY, NX = 1, 8
T = NY * NX
NKEYS, KEY_W = 3, 1         # key KEY_W of the bank is the engine's own W
NCOPIES = 3                 # wm_embed_signs_multi
NBITS = 4
OFF_ROWS, OFF_COLS, OFF_N = 42, 276, 2   # wm_detect_offsets: bank plane and offsets per axis
MAX_F, NSLOTS = 3, 3
SLOT_SYNC = -1
NBUF = 4
POOL_FRAMES = NBUF * MAX_F
NFRESH = 8                  # constant input frames (and as many separate grey bases)
ME, NVF = 0, 1

EMBEDS = ("embed", "embed_detect", "embed_signs", "embed_bits")
COPIES = ("embed_keys", "embed_signs_multi")
DETECTORS = ("detect", "detect_keys", "detect_offsets", "detect_tiles", "detect_keys_tiles", "detect_bits")
KINDS = EMBEDS + COPIES + DETECTORS + ("compute_mask", "sync")
GRAM_KERNELS = ("k_gram", "k_gram_ho", "k_gram_ho_checked", "k_gram_redo")

# the transitions tests/test_sequence_model.py wants covered (counted from the model alone)
TRANSITIONS = (
    "checked_trusted", "checked_redone", "promised_taken:detect", "ended_by_embed_on_another_slot", "ended_by_mask",
    "ended_by_copies", "slot_out_names_signs_output", "slot_out_unchanged_after_copies", "base_is_out_no_handover",
    "in_place_handover", "f1_no_handover", "not_taken_frames_differ", "not_taken_descriptor_differs", "ended_by_signs_on_its_own_slot")

# 48 sequences of 14 drawn calls: enough for every condition of tests/test_sequence_model.py (conditions, not measurements)
SEEDS = tuple(range(48))
N_OPS = 14


def overlap(a, b):
    return a[0] < b[0] + b[1] and b[0] < a[0] + a[1]


class ModelError(Exception):
    """a step the caller must not make (a race between slots, WM_MEM_SLOT_OUT without a matching output, ...)"""


class Model:
    """the slot state wm.h describes, advanced one step at a time by apply()"""

    def __init__(self, handover, checked, fused):
        self.handover, self.checked, self.fused = bool(handover), bool(checked), bool(fused)
        self.slots = [dict(last_out=None, last_by=None, copies_since=False, ho=None, reads=[], writes=[]) for _ in range(NSLOTS)]
        self.gram = collections.Counter()
        self.trusted = self.redone = 0
        self.transitions = collections.Counter()

    # -- helpers ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def slot_index(slot):
        return 0 if slot == SLOT_SYNC else slot

    def resolve(self, step, src):
        """the pool frames (start, n) behind an input, None for a constant input frame"""
        if src[0] == "fresh":
            return None
        if src[0] == "pool":
            return (src[1], src[2])
        s = self.slots[self.slot_index(step["slot"])]
        if s["last_out"] is None or s["last_out"][1] != step["F"]:
            raise ModelError("WM_MEM_SLOT_OUT: no matching embed output on this slot")
        return s["last_out"]

    def hazards(self, slot, reads, writes):
        """the other slots that must be synced before `slot` may read / write these frames"""
        out = []
        for t, s in enumerate(self.slots):
            if t == self.slot_index(slot):
                continue
            busy = any(overlap(w, x) for w in writes for x in s["reads"] + s["writes"]) or any(overlap(r, x) for r in reads for x in s["writes"])
            if busy:
                out.append(t)
        return out

    def _library_write(self, writer_slot, kind, rng, tr):
        """wm.h wm_set_handover: the library ends a hand-over whenever it writes that plane itself"""
        for t, s in enumerate(self.slots):
            if s["ho"] is not None and overlap((s["ho"]["start"], s["ho"]["F"]), rng):
                s["ho"] = None
                if kind in EMBEDS and t != writer_slot:
                    tr.append("ended_by_embed_on_another_slot")
                elif kind == "compute_mask":
                    tr.append("ended_by_mask")
                elif kind in COPIES:
                    tr.append("ended_by_copies")

    def _gram_of_detector(self, s, step, rng, tr, in_pair=False):
        """the detector side's Gram matrix: which path, and what it does to the slot's hand-over"""
        kind, F, ho = step["kind"], step["F"], s["ho"]
        by_slot_out = in_pair or step["src"][0] == "slot_out"
        wm_detect = kind in ("detect", "embed_detect")
        live = ho is not None and ho["F"] == F
        # wm_detect: the plane the slot's last wm_embed wrote (same pointer, pitch, frame stride, frames), sums no detector has
        # used yet, ME -> the checked hand-over.  (A WM_MEM_SLOT_OUT plane under a promise keeps the promised hand-over.)
        if wm_detect and self.checked and live and not ho["used"] and step["mask"] == ME and rng == (ho["start"], ho["F"]) and \
                not (by_slot_out and ho["promised"]):
            ho["used"] = True
            redone = sorted(ho["dirty"])
            self.gram["k_gram_ho_checked"] += 1
            self.gram["k_gram_redo"] += 1
            self.trusted += F - len(redone)
            self.redone += len(redone)
            tr.append("checked_redone" if redone else "checked_trusted")
            return "checked", ["redone" if f in redone else "trusted" for f in range(F)]
        if wm_detect and not by_slot_out and self.checked and ho is not None and not ho["used"] and step["mask"] == ME and rng is not None and \
                overlap(rng, (ho["start"], ho["F"])):
            tr.append("not_taken_frames_differ" if rng[0] == ho["start"] else "not_taken_descriptor_differs")
        # every detector: WM_MEM_SLOT_OUT under a promise (wm_set_handover, or the pair's own embed) takes the promised sums; a
        # second detector may take them again (they describe the plane, which by the promise has not changed)
        if by_slot_out and live and ho["promised"]:
            ho["used"] = True
            self.gram["k_gram_ho"] += 1
            if not in_pair:
                tr.append("promised_taken:" + kind)
            return "promised", ["promised"] * F
        self.gram["k_gram"] += 1
        return "ordinary", ["ordinary"] * F

    # -- one step ------------------------------------------------------------------------------------------------------------
    def apply(self, step):
        """advances the state by one step; returns what the model predicts for it"""
        kind, slot = step["kind"], step["slot"]
        si = self.slot_index(slot) if slot is not None else None
        s = self.slots[si] if slot is not None else None
        tr = []
        ann = dict(path=None, frame_paths=None, reads=[], writes=[], src_range=None)
        if kind == "sync":
            s["reads"], s["writes"] = [], []
            return ann
        if kind == "caller_write":
            if self.handover:
                raise ModelError("a caller's write under wm_set_handover breaks the promise")
            g = step["frame"]
            if any(overlap((g, 1), x) for t in self.slots for x in t["reads"] + t["writes"]):
                raise ModelError("caller write to a frame a slot still uses")
            for t in self.slots:
                if t["ho"] is not None and overlap((g, 1), (t["ho"]["start"], t["ho"]["F"])):
                    t["ho"]["dirty"].add(g - t["ho"]["start"])
            ann["writes"] = [(g, 1)]
            return ann
        F, mask = step["F"], step["mask"]
        fused = slot == SLOT_SYNC and F == 1 and self.fused and kind in ("embed", "detect", "embed_detect")
        if kind in EMBEDS:
            out = (step["out"], F)
            if step["variant"] in ("in_place", "base_is_out"):
                ann["reads"].append(out)
            ann["writes"].append(out)
        elif kind in COPIES:
            rng = self.resolve(step, step["src"])
            ann["src_range"] = rng
            if rng is not None:
                ann["reads"].append(rng)
            if step["out"] is not None:
                out = (step["out"], F * (NKEYS if kind == "embed_keys" else NCOPIES))
                if rng is not None and overlap(rng, out):
                    raise ModelError("copies overlap their input")
                ann["writes"].append(out)
        else:
            rng = self.resolve(step, step["src"])
            ann["src_range"] = rng
            if rng is not None:
                ann["reads"].append(rng)
            if kind == "compute_mask" and step["out"] is not None:
                out = (step["out"], F)
                if rng is not None and overlap(rng, out):
                    raise ModelError("mask output overlaps its input")
                ann["writes"].append(out)
        if self.hazards(slot, ann["reads"], ann["writes"]):
            raise ModelError("step %r races with slots %r" % (step, self.hazards(slot, ann["reads"], ann["writes"])))

        if kind in EMBEDS:
            # wm_embed / wm_embed_signs: the output becomes what WM_MEM_SLOT_OUT names; whatever hand-over the slot held is gone, and
            # so is that of any slot whose plane this output overwrites
            if s["ho"] is not None and kind in ("embed_signs", "embed_bits"):
                tr.append("ended_by_signs_on_its_own_slot")
            s["ho"] = None
            self._library_write(si, kind, out, tr)
            s["last_out"], s["last_by"], s["copies_since"] = out, kind, False
            ann["path"] = "fused" if fused else "ordinary"
            if kind in ("embed", "embed_detect") and not fused:
                promised = self.handover or kind == "embed_detect"
                want = promised or (self.checked and mask == ME)
                handed = want and F >= 2 and step["variant"] != "base_is_out"
                if want and F == 1:
                    tr.append("f1_no_handover")
                if want and F >= 2 and step["variant"] == "base_is_out":
                    tr.append("base_is_out_no_handover")
                if handed and step["variant"] == "in_place":
                    tr.append("in_place_handover")
                if handed:
                    s["ho"] = dict(promised=promised, used=False, F=F, start=out[0], dirty=set())
            if not fused and mask == ME:
                self.gram["k_gram"] += 1
            if kind == "embed_detect" and not fused:
                ann["path"], ann["frame_paths"] = self._gram_of_detector(s, step, out, tr, in_pair=True)
                # the pair's promise is the pair's own: without wm_set_handover nothing of it outlives the pair's detector
                if s["ho"] is not None and not self.handover:
                    s["ho"]["promised"], s["ho"]["used"] = False, True
        elif kind in COPIES:
            # wm_embed_keys / wm_embed_signs_multi: no hand-over of their own, WM_MEM_SLOT_OUT unchanged, overlapped hand-overs end
            if step["src"][0] == "slot_out":
                self._slot_out_read(s, tr)
            if ann["writes"]:
                self._library_write(si, kind, ann["writes"][0], tr)
            if s["last_out"] is not None:
                s["copies_since"] = True
            if mask == ME:
                self.gram["k_gram"] += 1
            ann["path"] = "ordinary"
        elif kind == "compute_mask":
            if step["src"][0] == "slot_out":
                self._slot_out_read(s, tr)
            if ann["writes"]:
                self._library_write(si, kind, ann["writes"][0], tr)
            if mask == ME:
                self.gram["k_gram"] += 1
            ann["path"] = "ordinary"
        else:
            if step["src"][0] == "slot_out":
                self._slot_out_read(s, tr)
            if fused:
                ann["path"] = "fused"
            else:
                ann["path"], ann["frame_paths"] = self._gram_of_detector(s, step, rng, tr)
        for name in tr:
            self.transitions[name] += 1
        ann["transitions"] = tr
        if slot == SLOT_SYNC:
            s["reads"], s["writes"] = [], []
        else:
            s["reads"] += ann["reads"]
            s["writes"] += ann["writes"]
        return ann

    @staticmethod
    def _slot_out_read(s, tr):
        if s["last_by"] in ("embed_signs", "embed_bits"):
            tr.append("slot_out_names_signs_output")
        if s["copies_since"]:
            tr.append("slot_out_unchanged_after_copies")


Sequence = collections.namedtuple("Sequence", "seed handover checked fused steps annotations model")


def _pick(rng, items, weights):
    w = np.asarray(weights, float)
    return items[int(rng.choice(len(items), p=w / w.sum()))]


# How the generator spends its draws.  A plain uniform draw almost never lines a detector up behind the embed whose hand-over it
# could take, so part of the steps AIM at a pending hand-over; the shares below were set so that the committed seed list meets the
# conditions of tests/test_sequence_model.py, and carry no other meaning.
KIND_WEIGHTS = dict(embed=8, embed_detect=3, embed_signs=2, embed_bits=2, embed_keys=2, embed_signs_multi=2, detect=4, detect_keys=2,
                    detect_offsets=2, detect_tiles=2, detect_keys_tiles=2, detect_bits=2, compute_mask=2, sync=2, caller_write=2)
EMBED_WEIGHT_DEFAULT_SWITCHES = 14   # wm_embed under the default switches (checked on, no promise): what a caller's write can meet
SLOT_WEIGHTS = ((0, 1, 2, SLOT_SYNC), (3, 3, 2.5, 1.5))
P_AIM = 0.6                          # a step behind a pending hand-over aims at it
# what an aimed step does, by the upper end of its share of a uniform draw
AIMED = ((0.45, "detector"),         # a detector on the hand-over's slot
         (0.56, "mask"),             # wm_compute_mask outputs over its plane
         (0.67, "copies"),           # wm_embed_keys / wm_embed_signs_multi copies over its plane
         (0.78, "embed_elsewhere"),  # an embed on another slot into its plane
         (0.88, "signs_over"),       # wm_embed_signs on its own slot over its plane, and a detector of that plane behind it
         (1.00, "caller_write"))     # (under wm_set_handover, where a caller must not write: a detector)
P_FOLLOW = 0.8                       # the step behind a caller's write / a signs_over step is the detector that has to notice
# the plane wm_detect names by pointer on a slot with a hand-over: the same plane, fewer frames, another first frame, any plane
POINTER = ((0.4, "same"), (0.7, "fewer_frames"), (0.95, "shifted"), (1.0, "any"))
# an aimed detector reads WM_MEM_SLOT_OUT with this probability (else a pointer)
P_SLOT_OUT = dict(other=0.85, detect_promised=0.45, detect_unpromised=0.25)


def _share(table, u):
    return next(name for top, name in table if u < top)


class _Draw:
    """the generator's state: the rng, the model it steps along, and the detector owed to the last step (`follow`)"""

    def __init__(self, seed):
        self.rng = np.random.default_rng([seed, 0x5E9])
        # half of the sequences run the default switches (checked on, no promise): the only ones a caller's write may meet a hand-over in
        self.handover, self.checked = ((False, True), (True, True), (False, True), (True, False), (False, True), (False, False))[seed % 6]
        self.fused = bool(self.rng.integers(2))
        self.m = Model(self.handover, self.checked, self.fused)
        self.follow = None   # (slot, first frame, frames, the hand-over must still be open): the plane the next detector should name
        w = dict(KIND_WEIGHTS)
        if self.checked and not self.handover:
            w["embed"] = EMBED_WEIGHT_DEFAULT_SWITCHES
        if self.handover:
            w["caller_write"] = 0
        self.kinds = list(KINDS) + ["caller_write"]
        self.weights = [w[k] for k in self.kinds]

    def integer(self, n):
        return int(self.rng.integers(n))

    def aimed(self, kind, slot):
        """(kind, slot, the hand-over aimed at or None, signs_over): part of the steps behind a pending hand-over aim at it"""
        rng, m = self.rng, self.m
        held = [(t, sl["ho"]) for t, sl in enumerate(m.slots) if sl["ho"] is not None and (sl["ho"]["promised"] or not sl["ho"]["used"])]
        if not held or rng.random() >= P_AIM:
            return kind, slot, None, False
        t, aim = held[self.integer(len(held))]
        what = _share(AIMED, rng.random())
        if what == "caller_write" and self.handover:
            what = "detector"
        if what == "detector":
            return _pick(rng, DETECTORS, [5, 1, 1, 1, 1, 1] if aim["promised"] else [5, 0, 0, 0, 0, 0.5]), t, aim, False
        if what == "mask":
            return "compute_mask", slot, aim, False
        if what == "copies":
            return _pick(rng, COPIES, [1, 1]), slot, aim, False
        if what == "embed_elsewhere":
            return _pick(rng, EMBEDS, [2, 1, 1, 1]), (t + 1 + self.integer(NSLOTS - 1)) % NSLOTS, aim, False
        if what == "signs_over":
            return _pick(rng, ["embed_signs", "embed_bits"], [1, 1]), t, aim, True
        return "caller_write", slot, aim, False

    def followed(self):
        """the plane (slot, (first frame, frames)) a detector owed to the last step should name, or None"""
        if self.follow is None:
            return None
        (t, start, F, live), self.follow = self.follow, None
        ho = self.m.slots[t]["ho"]
        if (not live or (ho is not None and not ho["used"])) and self.rng.random() < P_FOLLOW:
            return t, (start, F)
        return None

    def caller_write(self, step):
        """one pixel of one frame of an output plane; where a hand-over is open, mostly there"""
        rng, m = self.rng, self.m
        open_ = [t for t, sl in enumerate(m.slots) if sl["ho"] is not None and not sl["ho"]["used"]]
        if open_ and rng.random() < 0.8:
            t = open_[self.integer(len(open_))]
            ho = m.slots[t]["ho"]
            g = ho["start"] + self.integer(ho["F"])
            self.follow = (t, ho["start"], ho["F"], True)
        else:
            g = self.integer(POOL_FRAMES)
        step.update(slot=None, frame=g, row=self.integer(R), col=self.integer(C))

    def embed(self, step, F, aim, signs_over):
        step["variant"] = _pick(self.rng, ["base_is_in", "grey_base", "in_place", "base_is_out"], [3, 2, 2, 1.5])
        if signs_over:
            F, self.follow = aim["F"], (step["slot"], aim["start"], aim["F"], False)
        out = MAX_F * self.integer(3) if aim is None else aim["start"]
        step.update(F=F, out=out, x0=self.integer(NFRESH - F + 1), b0=self.integer(NFRESH - F + 1))

    def source(self, step, s, F, aim, exact):
        """the input plane of a detector, a copies call or wm_compute_mask: step["src"]; returns the frame count, which
        WM_MEM_SLOT_OUT and an aimed pointer set"""
        rng, kind = self.rng, step["kind"]
        choices, w = ["fresh", "pool"], [2, 3 if kind == "detect" else 1.5]
        if s["last_out"] is not None:
            choices.append("slot_out")
            w.append(4)
        how = _pick(rng, choices, w)
        if exact is not None:
            how, step["mask"] = "slot_out" if s["last_out"] == exact and rng.random() < 0.5 else "pool", ME
        elif aim is not None and kind not in DETECTORS:
            how = "fresh"
        elif aim is not None:
            p = P_SLOT_OUT["other"] if kind != "detect" else P_SLOT_OUT["detect_promised" if aim["promised"] else "detect_unpromised"]
            how = "slot_out" if rng.random() < p else "pool"
        if how == "slot_out":
            step["src"] = ("slot_out",)
            return s["last_out"][1]
        if how == "fresh":
            step["src"] = ("fresh", self.integer(NFRESH - F + 1))
            return F
        ho = s["ho"]
        where = _share(POINTER, rng.random())
        if exact is not None:
            start, F = exact
        elif kind == "detect" and ho is not None and where == "same":
            start, F = ho["start"], ho["F"]
        elif kind == "detect" and ho is not None and where == "fewer_frames":
            start, F = ho["start"], ho["F"] - 1
        elif kind == "detect" and ho is not None and where == "shifted":
            start, F = ho["start"] + 1, ho["F"] - 1
        else:
            start = MAX_F * self.integer(3) + self.integer(MAX_F - F + 1)
        step["src"] = ("pool", start, F)
        return F

    def outputs(self, step, F, aim):
        """where a copies call or wm_compute_mask writes: planes of its own (None), or pool frames that do not overlap its input"""
        rng, m, kind = self.rng, self.m, step["kind"]
        if kind in COPIES:
            n = F * (NKEYS if kind == "embed_keys" else NCOPIES)
            step["out"] = None
            if aim is not None or rng.random() < 0.6:
                start = MAX_F * self.integer((POOL_FRAMES - n) // MAX_F + 1)
                if aim is not None:
                    start = min(MAX_F * (aim["start"] // MAX_F), POOL_FRAMES - n)
                src = m.resolve(step, step["src"])
                if src is None or not overlap(src, (start, n)):
                    step["out"] = start
        elif kind == "compute_mask":
            step["out"], step["e_out"] = None, bool(rng.integers(2))
            if aim is not None or rng.random() < 0.35:
                start = MAX_F * self.integer(3) if aim is None else aim["start"]
                src = m.resolve(step, step["src"])
                if src is None or not overlap(src, (start, F)):
                    step["out"] = start
        elif kind == "detect_offsets":
            step["oy0"], step["ox0"] = self.integer(2), self.integer(3)

    def step(self):
        """one drawn call"""
        rng, m = self.rng, self.m
        kind = _pick(rng, self.kinds, self.weights)
        slot = _pick(rng, *SLOT_WEIGHTS)
        kind, slot, aim, signs_over = self.aimed(kind, slot)
        exact = None
        owed = self.followed()
        if owed is not None:
            kind, (slot, exact), aim, signs_over = "detect", owed, None, False
        s = m.slots[m.slot_index(slot)]
        step = dict(kind=kind, slot=slot, dseed=self.integer(1 << 30))
        if kind == "sync":
            if slot == SLOT_SYNC:
                step["slot"] = 0
        elif kind == "caller_write":
            self.caller_write(step)
        else:
            step["mask"] = _pick(rng, [ME, NVF], [3, 1])
            F = int(_pick(rng, [1, 2, 3], [3, 1, 1] if slot == SLOT_SYNC else [1, 2, 2]))
            if aim is not None and kind == "detect" and rng.random() < 0.7:
                step["mask"] = ME
            if kind in EMBEDS:
                self.embed(step, F, aim, signs_over)
            else:
                F = self.source(step, s, F, aim, exact)
                step["F"] = F
                step["b0"] = self.integer(NFRESH - F + 1)
                self.outputs(step, F, aim)
        return step


def generate(seed, n_ops=N_OPS):
    """a sequence of n_ops drawn calls (plus the syncs that keep slots from racing, and a final sync of every slot), with the
    model's prediction for every step.  Deterministic in (seed, n_ops)."""
    d = _Draw(seed)
    m, steps, anns = d.m, [], []

    def push(step):
        reads, writes = _accesses(m, step)
        busy = _users(m, step["frame"]) if step["kind"] == "caller_write" else m.hazards(step["slot"], reads, writes)
        for t in busy:
            sy = dict(kind="sync", slot=t, auto=True)
            steps.append(sy)
            anns.append(m.apply(sy))
        steps.append(step)
        anns.append(m.apply(step))

    for _ in range(n_ops):
        push(d.step())
    for t in range(NSLOTS):
        push(dict(kind="sync", slot=t, auto=True))
    return Sequence(seed, d.handover, d.checked, d.fused, steps, anns, m)


def _accesses(m, step):
    """what a step reads and writes, as Model.apply will judge it (the model is not advanced)"""
    kind = step["kind"]
    if kind in ("sync", "caller_write"):
        return [], []
    F, reads, writes = step["F"], [], []
    if kind in EMBEDS:
        writes.append((step["out"], F))
        if step["variant"] in ("in_place", "base_is_out"):
            reads.append((step["out"], F))
        return reads, writes
    rng = m.resolve(step, step["src"])
    if rng is not None:
        reads.append(rng)
    if step.get("out") is not None:
        writes.append((step["out"], F * (NKEYS if kind == "embed_keys" else NCOPIES if kind == "embed_signs_multi" else 1)))
    return reads, writes


def _users(m, frame):
    return [t for t, s in enumerate(m.slots) if any(overlap((frame, 1), x) for x in s["reads"] + s["writes"])]


def replay(seq):
    """the model run again over a sequence's steps: its annotations and its totals"""
    m = Model(seq.handover, seq.checked, seq.fused)
    return [m.apply(st) for st in seq.steps], m
