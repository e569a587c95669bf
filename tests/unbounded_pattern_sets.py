"""Pattern sets with unbounded quantifiers (krca.logdfa.compile_patterns(..., unbounded=True)) and the
texts their tests scan, shared by tests/test_logdfa_unbounded_cpu.py and
tests/test_gpu_log_unbounded.py.  Expected values always come from Python's ``re`` per line
(custom_pattern_sets.re_masks / re_hist), as in the fixed-length table tests."""
import re

import numpy as np

import custom_pattern_sets as S
from krca import logdfa


def _swap(base, name, rx):
    assert any(n == name for n, _ in base)
    return [(n, rx if n == name else p) for n, p in base]


U1 = _swap(S.S13, "exception", r"Exception.*at")
U2 = _swap(_swap(U1, "timeout", r"timed? ?out after \d+ ?m?s"), "api_error", r"StatusCode=5\d+")
U4 = [("err_timeout", r"error.*timeout"), ("retry", r"retry \d+/\d+"), ("xrun", r"x{3,}"), ("warn", r"warn[a-z]*:")]
# 36 symbols: rows of 64 columns, and close to the largest table the device holds
UB2 = _swap(_swap(S.SETS["B"], "api_error", r"StatusCode=5\d+"), "exception", r"Exception.*at")
# past the 1024-state limit: three more loops beside U2's; eight independent ".*"
U3 = _swap(_swap(_swap(U2, "oom_kill", r"Out of memory.*Killed|OOMKilled"), "dns_resolution",
                 r"lookup [\w.-]+: no such host"), "connection_refused", r"dial tcp .*: connection refused")
U8 = [("c" + c, f"w{c}{c}.*z{c}") for c in "abcdefgh"]

SETS = {"U1": U1, "U2": U2, "U4": U4, "UB2": UB2}
# (categories, symbols, states) as krca.logdfa gives them under CPython's re; a prototype of the
# construction with re as the classifier gave the same numbers before the compiler was written
SIZES = {"U1": (13, 31, 737), "U2": (13, 31, 719), "U4": (4, 18, 74), "UB2": (16, 36, 1002)}
TOO_LARGE = {"U3": (U3, 4408), "U8": (U8, 2814)}

_PICK = {r"\d": "7", r"\D": "x", r"\w": "w", r"\W": "-", r"\s": " ", r"\S": "s", ".": "_"}


def _member(atom):
    if atom in _PICK:
        return _PICK[atom]
    if atom.startswith("["):
        return next(chr(c) for c in range(33, 127) if re.fullmatch(atom, chr(c)))
    return atom[-1]  # a literal, escaped or not


def loop_examples(patterns, reps=(0, 1, 5, 40), gap=None):
    """One string per alternative and repeat count: every loop item taken `rep` times beyond its
    minimum (0: x{m,} at exactly m, x* at none).  gap: text put in place of the repeats of a '.'
    loop (other patterns' fragments inside a ".*")."""
    out = []
    for name, rx in patterns:
        for alt in logdfa.parse(name, rx, unbounded=True):
            for rep in reps:
                s = ""
                for item in alt:
                    if isinstance(item, str):
                        s += _member(item)
                    elif gap is not None and item[1] == ".":
                        s += gap
                    else:
                        s += _member(item[1]) * rep
                out.append(s)
    return list(dict.fromkeys(out))


def literals(patterns):
    """One matching string per alternative (loops taken once): what the block-edge, tile-boundary and
    container-end shapes of tests/test_gpu_log_tables.py are built from."""
    return loop_examples(patterns, reps=(1,))


def gap_examples(patterns):
    """Alternatives with a '.' loop, the gap holding fragments (whole, cut, nested) of other patterns."""
    lits = literals(patterns)
    out = []
    for k, g in enumerate((lits[0], lits[-1][:3], lits[1][2:] + " " + lits[0][:-1], "timeout at error", "٣" * 3,
                           "éKſ", lits[2] + lits[2])):
        out += loop_examples(patterns, reps=(1,), gap=g)[k % 2::2]
    return out


def fragment_fuzz(patterns, n_docs, seed):
    """custom_pattern_sets.fragment_fuzz over the loop examples: every example cut at a random point (or
    whole, case-flipped, with a Unicode case fold or Arabic-Indic digits put in), scattered over lines
    and containers with the same separators, multi-byte characters and fillers."""
    lits = loop_examples(patterns) + gap_examples(patterns)
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
                    a = re.sub(r"\d", lambda m: "٣", a)
                if r < 0.45:
                    cut = int(rng.integers(0, len(a) + 1))
                    a = a[:cut] if rng.random() < 0.5 else a[cut:]
                parts.append(a)
            elif r < 0.8:
                parts.append(S.SEPS[int(rng.integers(0, len(S.SEPS)))])
            else:
                parts.append(S.OTHER[int(rng.integers(0, len(S.OTHER)))] * int(rng.integers(1, 4)))
        docs.append("".join(parts))
    return docs


HAZARDS = ["ERROR … TİMEOUT", "error … tİmeout", "retry ٣٤٥/١ retry 12/", "retry 1/๑๒",
           "StatusCode=5٣٤٥ StatusCode=5", "StatusCode=5", "xx xxx", "xxXx", "warn: warnings: warné:", "WARNſ:",
           "Exception at", "Exceptionat", "exception at"[:9] + " AT", "at Exception", "timeout error", "errortimeout",
           "timed out after 5ms", "timeout after ٣٣ s", "tim out after 1s", "x" * 3, "x" * 2, ":", "warn",
           "Exception" + "é" * 50 + "at", "lookup a.b-c: no such host"]


# ---- long lines for U4: the wave-per-line kernel's 64 segments -----------------------------------------
def compose(nbytes, filler, pieces):
    """A line of exactly nbytes bytes: `pieces` [(byte offset, text)] in line order at exactly those
    offsets, filler code points between them (ASCII 'q' where a gap is no multiple of the filler's
    width, and at the line's end).  The segment size of the wave-per-line kernels is then
    ceil(nbytes / 64), as _long_line of tests/test_gpu_log_tables.py computes it from the line's length."""
    w, out, at = len(filler.encode()), [], 0
    for off, text in pieces:
        assert off >= at, (off, at)
        out.append("q" * ((off - at) % w) + filler * ((off - at) // w) + text)
        at = off + len(text.encode())
    assert at <= nbytes
    out.append(filler * ((nbytes - at) // w) + "q" * ((nbytes - at) % w))
    line = "".join(out)
    assert len(line.encode()) == nbytes
    return line


def seg_of(nbytes):
    return (nbytes + 63) // 64


PAIR_SIZES = (1025, 2048, 4099, 8000)


def _pairs():
    rng = np.random.default_rng(11)
    pairs = [(5, 5), (0, 0), (63, 63), (7, 8), (0, 1), (62, 63), (0, 63)]
    while len(pairs) < 27:
        i, j = sorted(int(v) for v in rng.integers(0, 64, 2))
        pairs.append((i, j))
    return pairs


def long_lines_u4():
    """[(tag, line)]: 1 025 to 8 000 bytes each, for set U4.
    - "error" in segment i and "timeout" in segment j (same, adjacent, (0, 63), 20 random pairs), and the
      same pairs with the two words swapped ("rev": no match of error.*timeout);
    - "retry <digits>/7" with the digit run crossing 1, 2 and 5 segment boundaries, and a 200-digit run;
    - "xxx" with 1 + 2 and 2 + 1 of its x's on either side of a boundary;
    each with 1-, 2- and 3-byte fillers (code points straddle the boundaries), the digit runs also in
    Arabic-Indic digits (2 bytes each).  A segment of a short line holds 17 bytes: the words of a pair in
    one segment are put 1 and 9 bytes into it."""
    out = []
    for filler in ("q", "é", "€"):
        for n, (i, j) in enumerate(_pairs()):
            nbytes = PAIR_SIZES[n % 4]
            seg = seg_of(nbytes)
            last = nbytes - 8  # segment 63 of a 1025-byte line is short: keep the words inside the line
            for tag, first, second in (("fwd", "error", "timeout"), ("rev", "timeout", "error")):
                o1 = min(i * seg + 1, last - 10)
                o2 = min(j * seg + (9 if i == j else 1), last)
                o2 = max(o2, o1 + len(first) + 1)
                out.append((f"{tag}-{i}-{j}-{len(filler.encode())}", compose(nbytes, filler, [(o1, first), (o2, second)])))
        for digit in ("7", "٣"):
            dw = len(digit.encode())
            for nbytes, k, crossed in ((2048, 9, 1), (2048, 30, 2), (4096, 17, 5), (1088, 3, None)):
                seg = seg_of(nbytes)
                nd = 200 if crossed is None else ((crossed - 1) * seg + 10 + dw - 1) // dw
                text = "retry " + digit * nd + "/7"
                out.append((f"retry-{crossed}-{len(filler.encode())}-{dw}", compose(nbytes, filler, [(k * seg - 11, text)])))
        for nbytes, k, before in ((1025, 1, 1), (3000, 40, 2), (8000, 63, 1), (2048, 17, 2)):
            out.append((f"x-{before}-{len(filler.encode())}", compose(nbytes, filler, [(k * seg_of(nbytes) - before, "xxx")])))
            out.append((f"x2-{before}-{len(filler.encode())}",
                        compose(nbytes, filler, [(k * seg_of(nbytes) - before, "xx"), (k * seg_of(nbytes) - before + 3, "x")])))
    return out


def worst_case_lines(nbytes=60000):
    """(with, without): "error" in the first segment and "timeout" in the last of one line of nbytes
    bytes -- the state error.* arms survives every boundary, so lane r of the carried kernel learns
    its entry state only in round r: 63 rounds, one serial walk of the line -- and the same line with
    the "error" overwritten."""
    seg = seg_of(nbytes)
    hit = compose(nbytes, "q", [(3, "error"), (63 * seg + 5, "timeout")])
    return hit, hit.replace("error", "qqqqq")
