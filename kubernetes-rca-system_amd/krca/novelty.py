"""Log-template novelty across stream windows (include/krca.h "template novelty").

``TemplateNovelty`` owns the device-resident table of (group, template hash) records and feeds it the
template histograms of one window at a time (NativeEngine.template_hist_device after
template_hist_finish); ``NoveltyReport`` is what a window returns: the templates never logged before
(NOVEL) and the known ones whose rate jumped (SURGE), and how many of each every container shows.

The numpy dtypes and ``home_slot`` mirror csrc/tmpl_novelty_layout.h (the tests compare them with the
library); they decode a state for ``records()`` and the snapshots.
"""
import collections
import ctypes

import numpy as np

from . import native

EMPTY_HASH = (1 << 64) - 1
EMPTY_GROUP = -1
NOVEL, SURGE = 1, 2
MAGIC = 0x314C504D54564F4E
MIN_CAPACITY, MAX_CAPACITY = 64, 1 << 30
INT32_MIN = -(1 << 31)

HEADER_DTYPE = np.dtype([("magic", "<u8"), ("capacity", "<i8"), ("n_claimed", "<i8"), ("n_live", "<i8"),
                         ("n_entries", "<i8"), ("n_touched", "<i4"), ("overflow", "<i4"), ("n_novel", "<i4"),
                         ("n_surge", "<i4"), ("n_reported", "<i4"), ("pad0", "<i4"), ("pad", "<u8", (24,))])
SLOT_DTYPE = np.dtype([("hash", "<u8"), ("group", "<i4"), ("first_win", "<i4"), ("last_win", "<i4"), ("n_win", "<i4"),
                       ("total", "<i8"), ("cur", "<u8"), ("first_doc", "<i4"), ("flags", "<i4"), ("pad", "<u8", (2,))])
REPORT_DTYPE = np.dtype([("hash", "<u8"), ("total_before", "<i8"), ("cur_lines", "<i8"), ("group", "<i4"),
                         ("flags", "<i4"), ("cur_docs", "<i4"), ("first_doc", "<i4"), ("first_win", "<i4"),
                         ("pad", "<i4")])
COUNT_NAMES = ("n_entries", "n_keys_touched", "n_novel", "n_surge", "n_reported", "n_live_slots")

_M64 = (1 << 64) - 1


def remap(h):
    """A template hash equal to the table's empty marker is counted under the marker - 1."""
    h = int(h) & _M64
    return EMPTY_HASH - 1 if h == EMPTY_HASH else h


def home_slot(h, group, capacity):
    """nov_home of csrc/tmpl_novelty_layout.h on the remapped hash: the slot a key's probe starts at."""
    x = remap(h) ^ (((int(group) & 0xFFFFFFFF) * 0x9E3779B97F4A7C15) & _M64)
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return x & (int(capacity) - 1)


def state_size(capacity):
    """nov_state_bytes: header | slots | touched list, rounded up to 256 bytes."""
    return (HEADER_DTYPE.itemsize + int(capacity) * (SLOT_DTYPE.itemsize + 4) + 255) // 256 * 256


def decode_state(raw):
    """raw state bytes (uint8 array) -> (header record, slots array)."""
    raw = np.ascontiguousarray(raw, np.uint8)
    hdr = raw[:HEADER_DTYPE.itemsize].view(HEADER_DTYPE)[0]
    cap = int(hdr["capacity"])
    if int(hdr["magic"]) != MAGIC or len(raw) != state_size(cap):
        raise ValueError("not a template-novelty state")
    return hdr, raw[HEADER_DTYPE.itemsize:HEADER_DTYPE.itemsize + cap * SLOT_DTYPE.itemsize].view(SLOT_DTYPE)


def live_records(raw):
    """{(group, hash): (first_win, last_win, n_win, total)} of the records with n_win > 0."""
    _, slots = decode_state(raw)
    s = slots[(slots["n_win"] > 0) & (slots["group"] != EMPTY_GROUP) & (slots["hash"] != np.uint64(EMPTY_HASH))]
    return {(int(g), int(h)): (int(a), int(b), int(c), int(t)) for g, h, a, b, c, t in
            zip(s["group"], s["hash"], s["first_win"], s["last_win"], s["n_win"], s["total"])}


NoveltyRecord = collections.namedtuple(
    "NoveltyRecord", "hash group flags cur_lines cur_docs first_doc first_win total_before")


def sort_records(records):
    """The order a report lists its records in: cur_lines descending, then group, then hash."""
    return sorted(records, key=lambda r: (-r.cur_lines, r.group, r.hash))


def records_of(rep):
    """REPORT_DTYPE array -> list of NoveltyRecord."""
    return [NoveltyRecord(int(r["hash"]), int(r["group"]), int(r["flags"]), int(r["cur_lines"]), int(r["cur_docs"]),
                          int(r["first_doc"]), int(r["first_win"]), int(r["total_before"])) for r in rep]


class NoveltyReport:
    """One window: .novel / .surged (host lists of NoveltyRecord, sorted by sort_records), .truncated
    (more records qualified than the report holds; the counts stay exact), .counts (dict over
    COUNT_NAMES), .doc_novel / .doc_surge (device int32 [D]), .window, .grown (the capacities the
    table was rehashed into during this update: before the window fitted, and after it when it left the
    table above 70 % load)."""

    def __init__(self, window, counts, records, doc_novel, doc_surge, grown=()):
        self.window = int(window)
        self.counts = dict(zip(COUNT_NAMES, (int(c) for c in counts)))
        recs = sort_records(records)
        self.novel = [r for r in recs if r.flags & NOVEL]
        self.surged = [r for r in recs if r.flags & SURGE]
        self.truncated = self.counts["n_reported"] > len(recs)
        self.doc_novel, self.doc_surge = doc_novel, doc_surge
        self.grown = tuple(grown)

    def top_containers(self, k=10):
        """The k containers with the most novel + surging templates this window (ties: the lowest id)
        -> [(container, n_novel, n_surge)], those with none left out."""
        if self.doc_novel is None or self.doc_novel.numel() == 0:
            return []
        both = self.doc_novel.long() + self.doc_surge.long()
        D = both.numel()
        key = both * D + (D - 1 - _arange_like(both))  # the lower id wins a tie
        top = key.topk(min(int(k), D)).indices.cpu().tolist()
        nov, sur = self.doc_novel.cpu().numpy(), self.doc_surge.cpu().numpy()
        return [(d, int(nov[d]), int(sur[d])) for d in top if nov[d] + sur[d] > 0]


def _arange_like(t):
    import torch
    return torch.arange(t.numel(), device=t.device, dtype=t.dtype)


class TemplateNovelty:
    """The novelty table of one stream on `engine`'s device.

    capacity: slots to start with (a power of two >= 64; the table grows when a window does not fit).
    ttl: windows after which an unseen template is forgotten (0 = never).  surge_ratio / surge_min: a
    known template surges when this window's lines reach surge_min and surge_ratio times its mean per
    window since first sight.  report_cap: the most records a window reports."""

    def __init__(self, engine, capacity=1 << 20, ttl=0, surge_ratio=4, surge_min=8, report_cap=4096):
        self.eng = engine
        self.capacity = int(capacity)
        self.ttl, self.surge_ratio, self.surge_min = int(ttl), int(surge_ratio), int(surge_min)
        self.report_cap = int(report_cap)
        if self.ttl < 0 or self.surge_ratio < 1 or self.surge_min < 1 or self.report_cap < 0:
            raise ValueError("TemplateNovelty: ttl, report_cap >= 0 and surge_ratio, surge_min >= 1")
        self.last_window = -1
        self.state = self._new_state(self.capacity)

    def params(self):
        return dict(ttl=self.ttl, surge_ratio=self.surge_ratio, surge_min=self.surge_min, report_cap=self.report_cap)

    # -- the table -------------------------------------------------------------------------------
    def _new_state(self, capacity, init=True):
        e = self.eng
        n = e.lib.krca_template_novelty_state_size(capacity)
        if n <= 0:
            raise ValueError(f"TemplateNovelty: capacity {capacity} is no power of two in [{MIN_CAPACITY}, 2^30]")
        st = e.torch.empty(n, dtype=e.torch.uint8, device=e.device)
        if init:
            native._check(e.lib.krca_template_novelty_init(e.ptr(st), capacity, e._stream()), "krca_template_novelty_init")
        return st

    def rehash(self, new_capacity, min_last_window=INT32_MIN):
        """Move the records with last_win >= min_last_window into a table of new_capacity slots."""
        e = self.eng
        st = self._new_state(int(new_capacity), init=False)
        native._check(e.lib.krca_template_novelty_rehash(e.ptr(self.state), e.ptr(st), int(new_capacity),
                                                         int(max(min_last_window, INT32_MIN)), e._stream()),
                      "krca_template_novelty_rehash")
        self.state, self.capacity = st, int(new_capacity)

    def header(self):
        return self.state[:HEADER_DTYPE.itemsize].cpu().numpy().view(HEADER_DTYPE)[0]

    def records(self):
        """The live records on the host: {(group, hash): (first_win, last_win, n_win, total)}."""
        _, rows = self._claimed()
        s = rows[rows["n_win"] > 0]
        return {(int(g), int(h)): (int(a), int(b), int(c), int(t)) for g, h, a, b, c, t in
                zip(s["group"], s["hash"], s["first_win"], s["last_win"], s["n_win"], s["total"])}

    def _claimed(self):
        """-> (slot indices int64 [n], their slots as a host SLOT_DTYPE array) of the slots holding a key."""
        torch = self.eng.torch
        lo = HEADER_DTYPE.itemsize
        slots = self.state[lo:lo + self.capacity * SLOT_DTYPE.itemsize].view(self.capacity, SLOT_DTYPE.itemsize)
        group = slots.view(torch.int32)[:, SLOT_DTYPE.fields["group"][1] // 4]
        idx = torch.nonzero(group != EMPTY_GROUP).view(-1)
        rows = slots[idx].cpu().numpy().reshape(-1).view(SLOT_DTYPE)
        return idx.cpu().numpy(), rows

    def _double(self, window):
        if 2 * self.capacity > MAX_CAPACITY:
            raise native.KrcaError("template novelty: the table cannot grow past 2^30 slots")
        self.rehash(2 * self.capacity, window - self.ttl if self.ttl > 0 else INT32_MIN)

    def _grow(self, window, compacted):
        """Make room: once per window drop what the ttl has expired (a rehash at the same size, which
        also reclaims the absent slots a failed window left) and double only if the table is still more
        than half full; a window that fails again after that doubles unconditionally."""
        if self.ttl > 0 and not compacted:
            self.rehash(self.capacity, window - self.ttl)
            if 2 * int(self.header()["n_claimed"]) <= self.capacity:
                return
        self._double(window)

    # -- one window ------------------------------------------------------------------------------
    def update(self, templates, doc_line0, group=None, window=None, report=True, docs=True):
        """templates: NativeEngine.template_hist_device's dict (after template_hist_finish), or any dict
        of device tensors tmpl_hash int64 / tmpl_count int32 [L] and n_templates int32 [D]; doc_line0
        int64 [D]; group int32 [D] or None (every container in group 0).  window: defaults to the last
        one + 1 and must increase strictly.  report=False learns the window and reports nothing.
        docs=False skips the per-container counts.  -> NoveltyReport."""
        e, torch = self.eng, self.eng.torch
        w = self.last_window + 1 if window is None else int(window)
        if w <= self.last_window or w < 0 or w >= (1 << 31):
            raise ValueError(f"TemplateNovelty.update: window {w} does not follow window {self.last_window}")
        th, tc, nt = templates["tmpl_hash"], templates["tmpl_count"], templates["n_templates"]
        D, L = int(nt.numel()), int(min(th.numel(), tc.numel()))
        if doc_line0.numel() != D or (group is not None and group.numel() != D):
            raise ValueError("TemplateNovelty.update: n_templates, doc_line0 and group must have one element per container")
        if group is not None and group.dtype != torch.int32:
            raise ValueError("TemplateNovelty.update: group must be int32")
        cap = self.report_cap
        rep = torch.empty(max(cap, 1) * REPORT_DTYPE.itemsize, dtype=torch.uint8, device=e.device)
        dn = torch.empty(D, dtype=torch.int32, device=e.device) if docs else None
        ds = torch.empty(D, dtype=torch.int32, device=e.device) if docs else None
        counts = (ctypes.c_int64 * 6)()
        grown = []
        compacted = False
        while True:
            rc = e.lib.krca_template_novelty_update(
                e.ptr(self.state), e.ptr(th), e.ptr(tc), L, e.ptr(nt), e.ptr(doc_line0),
                e.ptr(group) if group is not None else None, D, w, self.ttl, self.surge_ratio, self.surge_min,
                1 if report else 0, e.ptr(rep), cap, e.ptr(dn) if docs and D else None, e.ptr(ds) if docs and D else None,
                counts, e._stream())
            if rc != native.KRCA_ENOMEM:
                native._check(rc, "krca_template_novelty_update")
                break
            self._grow(w, compacted)
            compacted = True
            grown.append(self.capacity)
        self.last_window = w
        if 10 * int(counts[5]) > 7 * self.capacity:
            # above 70 % load linear probing walks long chains: make room before the next window, not after
            # it has failed.  After a window that fitted, n_live_slots is the number of slots holding a key
            # (absent slots are left only by a failed window, and that one was followed by a rehash).
            self._grow(w, False)
            grown.append(self.capacity)
        n = min(int(counts[4]), cap)
        recs = records_of(rep[:n * REPORT_DTYPE.itemsize].cpu().numpy().view(REPORT_DTYPE)) if n else []
        return NoveltyReport(w, list(counts), recs, dn, ds, grown)

    def example(self, record, scan):
        """The text of the first line of container record.first_doc whose template hash is the record's:
        how a template is shown to a person.  scan: the window's push_logs / log_scan_device dict with
        its "templates" (the per-line hashes).  None when the container holds no such line."""
        d = int(record.first_doc)
        lo = int(scan["doc_line0"][d].item())
        n = int(scan["doc_lines"][d].item())
        h = scan["templates"]["hash"][lo:lo + n].cpu().numpy().view(np.uint64)
        h = np.where(h == np.uint64(EMPTY_HASH), np.uint64(EMPTY_HASH - 1), h)
        hit = np.flatnonzero(h == np.uint64(record.hash))
        if len(hit) == 0:
            return None
        li = lo + int(hit[0])
        s, t = int(scan["line_start"][li].item()), int(scan["line_end"][li].item())
        return bytes(scan["text"][s:t].cpu().numpy()).decode("utf-8", "replace")

    # -- snapshots ---------------------------------------------------------------------------------
    def state_dict(self):
        """The table as host arrays: the slots that hold a key (raw bytes of csrc/tmpl_novelty_layout.h:
        plain data, no pointers) with their positions, the header, the capacity and the last window.  Empty
        slots and the touched list are not stored: the size follows the keys, not the capacity, and equal
        tables give equal bytes."""
        idx, rows = self._claimed()
        return dict(novelty_slots=rows.view(np.uint8).reshape(-1, SLOT_DTYPE.itemsize), novelty_index=idx.astype(np.int64),
                    novelty_header=self.state[:HEADER_DTYPE.itemsize].cpu().numpy(),
                    novelty_meta=np.array([self.capacity, self.last_window], np.int64))

    def load_state_dict(self, st):
        cap, last = (int(v) for v in np.asarray(st["novelty_meta"], np.int64))
        hdr = np.ascontiguousarray(st["novelty_header"], np.uint8)
        rows = np.ascontiguousarray(st["novelty_slots"], np.uint8)
        idx = np.ascontiguousarray(st["novelty_index"], np.int64)
        h = hdr.view(HEADER_DTYPE)[0]
        if hdr.shape != (HEADER_DTYPE.itemsize,) or int(h["magic"]) != MAGIC or int(h["capacity"]) != cap or \
                rows.shape != (len(idx), SLOT_DTYPE.itemsize) or (len(idx) and (idx.min() < 0 or idx.max() >= cap)):
            raise ValueError("template novelty snapshot: header, slots and capacity do not fit together")
        e, torch = self.eng, self.eng.torch
        state = self._new_state(cap)  # every slot empty, then the stored ones in their places
        lo = HEADER_DTYPE.itemsize
        if len(idx):
            state[lo:lo + cap * SLOT_DTYPE.itemsize].view(cap, SLOT_DTYPE.itemsize)[torch.from_numpy(idx).to(e.device)] = \
                torch.from_numpy(rows).to(e.device)
        state[:lo] = torch.from_numpy(hdr).to(e.device)
        self.state, self.capacity, self.last_window = state, cap, last
