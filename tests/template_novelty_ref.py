"""Host restatement of the log-template novelty table (include/krca.h "template novelty", DESIGN.md
§3.18): a dict of records, one window at a time, no capacity.  It is the definition the device is
compared with bit for bit; every quantity is a Python int.

The entries of a window come from the four template arrays exactly as the header defines them: for
every container d with group[d] >= 0 and j < n_templates[d], (group[d], tmpl_hash[doc_line0[d] + j],
tmpl_count[doc_line0[d] + j]); a count <= 0 or a slot outside [0, len(tmpl_hash)) is no entry.
"""
import numpy as np

EMPTY_HASH = (1 << 64) - 1
NOVEL, SURGE = 1, 2


def remap(h):
    """A hash equal to the table's empty marker is counted under the marker - 1."""
    h = int(h)
    return EMPTY_HASH - 1 if h == EMPTY_HASH else h


def entries(tmpl_hash, tmpl_count, n_templates, doc_line0, group=None):
    """-> list of (d, group, remapped hash, count) in container order."""
    th = np.asarray(tmpl_hash).view(np.uint64) if np.asarray(tmpl_hash).dtype == np.int64 else np.asarray(tmpl_hash, np.uint64)
    tc = np.asarray(tmpl_count)
    out = []
    L = len(th)
    for d, (n, o) in enumerate(zip(np.asarray(n_templates).tolist(), np.asarray(doc_line0).tolist())):
        g = 0 if group is None else int(group[d])
        if g < 0:
            continue
        for j in range(max(n, 0)):
            i = o + j
            if 0 <= i < L and int(tc[i]) > 0:
                out.append((d, g, remap(th[i]), int(tc[i])))
    return out


class Window:
    """What one update returns: counts[6], the report as a sorted list of tuples (hash, group, flags,
    cur_lines, cur_docs, first_doc, first_win, total_before), doc_novel / doc_surge int32 [D]."""

    def __init__(self, counts, report, doc_novel, doc_surge):
        self.counts, self.report, self.doc_novel, self.doc_surge = counts, report, doc_novel, doc_surge


class NoveltyRef:
    def __init__(self, ttl=0, surge_ratio=4, surge_min=8):
        self.ttl, self.surge_ratio, self.surge_min = int(ttl), int(surge_ratio), int(surge_min)
        self.rec = {}  # (group, hash) -> [first_win, last_win, n_win, total]

    def records(self):
        """{(group, hash): (first_win, last_win, n_win, total)} of the records with n_win > 0."""
        return {k: tuple(v) for k, v in self.rec.items() if v[2] > 0}

    def compact(self, min_last_window):
        """What krca_template_novelty_rehash keeps."""
        self.rec = {k: v for k, v in self.rec.items() if v[2] > 0 and v[1] >= min_last_window}

    def update(self, tmpl_hash, tmpl_count, n_templates, doc_line0, group, window, report=True, cap=None):
        w = int(window)
        D = len(n_templates)
        ent = entries(tmpl_hash, tmpl_count, n_templates, doc_line0, group)
        cur = {}  # key -> [lines, docs, first_doc]
        for d, g, h, c in ent:
            a = cur.setdefault((g, h), [0, 0, d])
            a[0] += c
            a[1] += 1
            a[2] = min(a[2], d)
        flags = {}
        rep = []
        for key, (lines, docs, first_doc) in cur.items():
            r = self.rec.get(key)
            absent = r is None or r[2] == 0 or (self.ttl > 0 and r[1] < w - self.ttl)
            total = 0 if absent else r[3]
            first_win = w if absent else r[0]
            f = 0
            if report:
                if absent:
                    f = NOVEL
                elif lines >= self.surge_min and lines * (w - first_win) >= self.surge_ratio * total:
                    f = SURGE
            flags[key] = f
            if f:
                rep.append((key[1], key[0], f, lines, docs, first_doc, first_win, total))
            self.rec[key] = [first_win, w, 1 if absent else r[2] + 1, total + lines]
        doc_novel, doc_surge = np.zeros(D, np.int32), np.zeros(D, np.int32)
        for d, g, h, _ in ent:
            doc_novel[d] += flags[(g, h)] == NOVEL
            doc_surge[d] += flags[(g, h)] == SURGE
        n_novel = sum(1 for f in flags.values() if f == NOVEL)
        n_surge = sum(1 for f in flags.values() if f == SURGE)
        counts = [len(ent), len(cur), n_novel, n_surge, len(rep), len(self.records())]
        return Window(counts, sorted(rep), doc_novel, doc_surge)
