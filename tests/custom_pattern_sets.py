"""Pattern sets of the run-time log pattern compiler's tests (krca/logdfa.py), shared by the CPU
and GPU test modules and by tests/golden/capture_custom_patterns.py, plus the line generators the
tests scan.  Expected values always come from Python's ``re`` (the reference's definition)."""
import re

import numpy as np

from krca.patterns import ERROR_PATTERNS

S13 = [tuple(p) for p in ERROR_PATTERNS]


def _swap(name, rx):
    return [(n, rx if n == name else p) for n, p in S13]


SETS = {
    "S13": S13,
    # one category edited; one removed; three small ones (ncat = 3); three added (ncat = 16, > 31 symbols)
    "A": _swap("timeout", r"(deadline exceeded|context canceled|timed out)"),
    "D": [p for p in S13 if p[0] != "timeout"],
    "C": [("jvm", r"(java.lang.OutOfMemoryError|GC overhead limit exceeded)"),
          ("http5xx", r"(HTTP/1.1\" 5\d\d|status=5\d\d)"),
          ("zk", r"(zookeeper session expired|KeeperErrorCode)")],
    "B": S13 + [("quota", r"(quota exceeded|rate limit|429 Too Many Requests)"),
                ("tls", r"(x509: certificate|handshake failure|TLS handshake timeout)"),
                ("disk", r"(No space left on device|disk pressure|I/O error)")],
    # every supported construct: bracket class, negated class, \w, \s, \D, {3}, {1,2}, ?, escaped . and (
    "E": [("cls", r"[a-c][^x-z]z{3}"), ("word", r"id=\w\s\D"), ("quant", r"ab{1,2}c?\.\("), ("plain", r"plain|other"),
          ("digits", r"(n=\d{1,2};|[0-9a-f]{4}-\S)")],
}
# (categories, symbols, states) of each set: A-D as measured for the issue with the build-time
# generator, E as the run-time compiler gives it (within the limits of 16 / 63 / 1024)
SIZES = {"S13": (13, 31, 394), "A": (13, 31, 417), "D": (12, 31, 381), "C": (3, 31, 130), "B": (16, 36, 543)}

# a set whose longest alternative is 40 code points (the long-line test: warm-up 39, not 23)
LONG40 = [("long40", "(" + "abcdefghij" * 4 + "|zq)"), ("digit", r"x\d\dy")]


def re_masks(patterns, text):
    """Per line of text.splitlines(): the category mask of re.search(regex, line, re.IGNORECASE)."""
    comp = [re.compile(p, re.IGNORECASE) for _, p in patterns]
    return [sum(1 << c for c, r in enumerate(comp) if r.search(line)) for line in text.splitlines()]


def re_hist(patterns, text):
    """(n_lines, hist[ncat], examples[ncat] = first three matching lines) as the reference's loop."""
    lines = text.splitlines()
    comp = [re.compile(p, re.IGNORECASE) for _, p in patterns]
    hist, ex = [], []
    for r in comp:
        hit = [ln for ln in lines if r.search(ln)]
        hist.append(len(hit))
        ex.append(hit[:3])
    return len(lines), hist, ex


def literals(patterns):
    """One literal string per alternative of every pattern (classes and escapes replaced by a member)."""
    from krca import logdfa
    pick = {r"\d": "7", r"\D": "x", r"\w": "w", r"\W": "-", r"\s": " ", r"\S": "s", ".": "_"}
    out = []
    for name, rx in patterns:
        for alt in logdfa.parse(name, rx):
            s = ""
            for atom in alt:
                if atom in pick:
                    s += pick[atom]
                elif atom.startswith("["):
                    s += next(chr(c) for c in range(33, 127) if re.fullmatch(atom, chr(c)))
                else:
                    s += atom[-1]  # a literal, escaped or not
            out.append(s)
    return out


SEPS = ["\n", "\r", "\r\n", "\x0b", "\x0c", "\x1c", "\x1d", "\x1e", "\x85", "\u2028", "\u2029", ""]
OTHER = ["\u00e9", "\u0130", "\u212a", "\u017f", "x", " ", "0", "a" * 13, "q" * 40, "\u0663", "\u0e51",
         "id=\u00e9\u2003x", "id=\u4e2d\u00a0-", "\u00df", "\U0001d7d8"]


def fragment_fuzz(patterns, n_docs, seed):
    """Containers built as tests/test_gpu_kernels.py::test_log_scan_fragment_fuzz builds them: every
    alternative cut at a random point (or whole, or case-flipped, or with a Unicode case fold put in),
    its halves scattered over lines and containers with separators, multi-byte characters, Arabic-Indic
    / Thai / mathematical digits (\\d), non-ASCII \\w / \\s code points and fillers of random length."""
    lits = literals(patterns)
    rng = np.random.default_rng(seed)
    folds = {"k": "\u212a", "K": "\u212a", "s": "\u017f", "S": "\u017f", "i": "\u0130", "I": "\u0130"}
    docs = []
    for _ in range(n_docs):
        parts = []
        for _ in range(int(rng.integers(0, 12))):
            r = rng.random()
            if r < 0.6:
                a = lits[int(rng.integers(0, len(lits)))]
                v = rng.random()
                if v < 0.2:
                    a = a.swapcase()
                elif v < 0.35:
                    a = "".join(folds.get(ch, ch) if rng.random() < 0.3 else ch for ch in a)
                elif v < 0.45:
                    a = re.sub(r"\d", lambda m: "\u0663", a)
                if r < 0.45:
                    cut = int(rng.integers(0, len(a) + 1))
                    a = a[:cut] if rng.random() < 0.5 else a[cut:]
                parts.append(a)
            elif r < 0.8:
                parts.append(SEPS[int(rng.integers(0, len(SEPS)))])
            else:
                parts.append(OTHER[int(rng.integers(0, len(OTHER)))] * int(rng.integers(1, 4)))
        docs.append("".join(parts))
    return docs
