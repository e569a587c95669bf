"""Run-time compiler of log pattern sets into the device matcher's tables.

``compile_patterns(patterns)`` turns an ordered sequence of ``(name, regex)`` pairs into a
:class:`LogTables`: the same tables ``csrc/gen_log_dfa.py`` builds offline for the 13 shipped
patterns (``ascii_sym``, ``ranges``, ``trans``, ``out`` ...), for any pattern set inside the
supported subset, plus ``image()``, the flat buffer of include/krca.h that
``krca_log_tables_upload`` takes.

Semantics are the reference's (ref:agents/logs_agent.py:147-149): line ``l`` of
``str.splitlines()`` is in category ``c`` iff ``re.search(regex_c, l, re.IGNORECASE)``.  Code
points are grouped into symbols by asking CPython's own ``re`` which atoms match them, so the
tables are exact for the running interpreter's Unicode data.

Supported syntax: every regex must expand to a finite set of alternatives of single-code-point
atoms -- top-level ``|`` (optionally inside ONE outer pair of parentheses); atoms: a literal,
``.``, ``\\d \\D \\w \\W \\s \\S``, an escaped metacharacter, a bracket class with ranges and
negation; quantifiers ``{n}``, ``{m,n}`` and ``?`` on one atom (expanded into alternatives).
By default the alternatives are fixed-length and everything else raises
:class:`PatternsUnsupported`: ``* + {m,}``, anchors, ``\\b``, nested groups, back-references,
look-around, inline flags, a regex ``re.compile`` rejects.

``compile_patterns(patterns, unbounded=True)`` also takes ``*``, ``+``, ``{m,}`` and ``{,}`` on one
atom: ``x{m,}`` is m copies of ``x`` followed by a LOOP ITEM on ``x``, a position of the alternative
that a matching code point does not leave.  Still refused: a quantifier on anything but one atom,
the lazy and possessive forms, and an alternative that can match the empty string (``a*``,
``x*y?``: it matches every line).  What loops cost is states, not symbols: a ``\\d+``-style loop
whose atom the next atom excludes is nearly free, but ``.*`` between two literals keeps "the
first literal was seen" alive beside every position of every other pattern and roughly doubles
the product DFA.  One ``.*`` fits beside the 13 shipped patterns (737 states of 1024), two do
not; the "states" limit then raises with the measured count.

Long lines: the device's wave-per-line kernel starts each of its 64 segments from the start state
after a warm-up of ``warm`` code points.  For a fixed-length set ``warm`` is the longest
alternative minus one and that is exact.  A set with loop items has no such bound: its image
carries ``FLAG_CARRY`` and the launcher takes ``log_dfa_long_carry_rt``, which hands each segment's
exit state to the next lane and re-walks until nothing changes; ``warm`` (loops counted at their
minimum, at most 63) is then only the speculation's warm-up.  :func:`simulate_segments` restates
that kernel in Python.
"""
import re
import struct
import unicodedata
import warnings

import numpy as np

from .patterns import PatternsChanged, pattern_digest

MAXCP = 0x110000
SEP = 0xFF

# limits of the device walk (include/krca.h KRCA_LOG_MAX_*)
MAX_NCAT = 16      # category bits 0-15 and example bits 16-31 of line_mask
MAX_NSYM = 63      # 64 columns per state row, the last is the identity column
MAX_NSTATE = 1024  # 10 bits of a 16-bit table entry
MAX_NRANGE = 1024
MAX_ALT_LEN = 64   # code points per alternative
MAX_ALTS = 256     # alternatives in the set after expansion

IMAGE_MAGIC = 0x544C524B  # "KRLT"
IMAGE_VERSION = 1
IMAGE_HEADER = struct.Struct("<8IQ2I")  # magic version ncat nsym nstate nrange warm other | digest | nbytes flags
FLAG_CARRY = 1     # header flag bit 0 (KRCA_LOG_FLAG_CARRY): long lines need the state carried between segments


class PatternsUnsupported(PatternsChanged):
    """A pattern set outside the subset (or the limits) the run-time compiler handles."""


# ---- parsing ---------------------------------------------------------------------------------
_CLASS_ESCAPES = "dDwWsS"
_BRACES = re.compile(r"\{(\d*)(,(\d*))?\}")
_GROUP_KINDS = (("(?=", "look-ahead"), ("(?!", "look-ahead"), ("(?<=", "look-behind"), ("(?<!", "look-behind"),
                ("(?P=", "back-reference"), ("(?:", "nested group"), ("(?P<", "nested group"), ("(?#", "comment group"),
                ("(?(", "conditional group"), ("(?", "inline flags"))


def _bad(name, what):
    raise PatternsUnsupported(f"log category {name!r}: {what} is not supported by the run-time pattern compiler "
                              f"(krca/logdfa.py lists the supported subset)")


def _bracket_end(rx, i):
    """index of the ']' closing the class that opens at rx[i] == '['."""
    j = i + 1
    if j < len(rx) and rx[j] == "^":
        j += 1
    if j < len(rx) and rx[j] == "]":
        j += 1
    while j < len(rx) and rx[j] != "]":
        j += 2 if rx[j] == "\\" else 1
    return j


def _tokens(name, rx, unbounded=False):
    """regex -> tokens ('atom', regex of one code point) | ('q', m, n) | ('|',) | ('(',) | (')',);
    n is None for an unbounded quantifier (taken under ``unbounded`` only)."""
    out, i, n = [], 0, len(rx)
    while i < n:
        ch = rx[i]
        if ch == "\\":
            e = rx[i + 1]
            if e in _CLASS_ESCAPES:
                out.append(("atom", "\\" + e))
            elif e.isdigit():
                _bad(name, f"back-reference or octal escape '\\{e}'")
            elif e in "bB":
                _bad(name, f"word boundary '\\{e}'")
            elif e in "AZ":
                _bad(name, f"anchor '\\{e}'")
            elif e.isalnum():
                _bad(name, f"escape '\\{e}'")
            else:
                out.append(("atom", re.escape(e)))
            i += 2
        elif ch == "[":
            j = _bracket_end(rx, i)
            out.append(("atom", rx[i:j + 1]))
            i = j + 1
        elif ch == "(":
            if rx.startswith("(?", i):
                _bad(name, next(k for p, k in _GROUP_KINDS if rx.startswith(p, i)) + f" '{rx[i:i + 4]}'")
            out.append(("(",))
            i += 1
        elif ch in ")|":
            out.append((ch,))
            i += 1
        elif ch in "^$":
            _bad(name, f"anchor '{ch}'")
        elif ch in "*+" and not unbounded:
            _bad(name, f"unbounded quantifier '{ch}'")
        elif ch in "*+?" or (ch == "{" and rx[i + 1:i + 2] != "}" and _BRACES.match(rx, i)):
            if ch != "{":
                q, j = {"?": (0, 1), "*": (0, None), "+": (1, None)}[ch], i + 1
            else:  # sre's reading of braces: {m} {m,n} {,n}; {m,} and {,} have no upper bound
                m = _BRACES.match(rx, i)
                j = m.end()
                lo, comma, hi = m.group(1), m.group(2), m.group(3)
                if comma and not hi and not unbounded:
                    _bad(name, f"unbounded quantifier '{rx[i:j]}'")
                q = (int(lo or 0), (int(hi) if hi else None) if comma else int(lo))
            if not out or out[-1][0] != "atom":
                _bad(name, f"quantifier '{rx[i:j]}' on anything but one atom")
            if j < n and rx[j] in "?+":
                _bad(name, f"lazy or possessive quantifier '{rx[i:j + 1]}'")
            out.append(("q",) + q)
            i = j
        elif ch == ".":
            out.append(("atom", "."))
            i += 1
        else:
            out.append(("atom", re.escape(ch)))
            i += 1
    return out


def parse(name, rx, unbounded=False):
    """One category's regex -> list of alternatives, each a tuple of atom regexes.  Under ``unbounded``
    an item of an alternative may also be a loop item ``("*", atom regex)``."""
    if not isinstance(rx, str):
        _bad(name, f"a pattern of type {type(rx).__name__}")
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            re.compile(rx, re.IGNORECASE)
    except (re.error, RecursionError, OverflowError) as e:
        _bad(name, f"a regex re.compile rejects ({e})")
    toks = _tokens(name, rx, unbounded)
    if toks and toks[0] == ("(",):  # one outer pair of parentheses
        depth, close = 0, None
        for k, t in enumerate(toks):
            depth += t == ("(",)
            depth -= t == (")",)
            if depth == 0:
                close = k
                break
        if close == len(toks) - 1:
            toks = toks[1:-1]
    if any(t[0] in "()" for t in toks):
        _bad(name, "nested group (parentheses other than one outer pair)")
    alts, cur = [], [()]
    for k, t in enumerate(toks + [("|",)]):
        if t[0] == "|":
            alts.extend(cur)
            cur = [()]
        elif t[0] == "atom":
            m, n = (toks[k + 1][1:] if k + 1 < len(toks) and toks[k + 1][0] == "q" else (1, 1))
            if n is None:  # x{m,}: m copies of x, then a loop item on x
                if m > MAX_ALT_LEN:
                    _bad(name, f"an alternative of more than {MAX_ALT_LEN} code points (a repeat of {m})")
                cur = [a + (t[1],) * m + (("*", t[1]),) for a in cur]
                continue
            if m > n:
                _bad(name, f"quantifier {{{m},{n}}} with min > max")
            if n > MAX_ALT_LEN:
                _bad(name, f"an alternative of more than {MAX_ALT_LEN} code points (a repeat of {n})")
            cur = [a + (t[1],) * r for a in cur for r in range(m, n + 1)]
            if len(cur) + len(alts) > MAX_ALTS:
                _bad(name, f"more than {MAX_ALTS} alternatives after expanding quantifiers ({len(cur) + len(alts)}+)")
    alts = list(dict.fromkeys(alts))
    for a in alts:
        if not any(isinstance(it, str) for it in a):  # nothing, or loop items only
            _bad(name, "an empty alternative (it matches every line)")
        ncp = sum(isinstance(it, str) for it in a)  # loop items count at their minimum, none
        if ncp > MAX_ALT_LEN:
            _bad(name, f"an alternative of {ncp} code points (at most {MAX_ALT_LEN})")
    return alts


# ---- code point classes ------------------------------------------------------------------------
_ALL = None     # every code point once, surrogates included (re and str handle them)
_SEPS = None    # str.splitlines separators of this interpreter
_ATOM_CP = {}   # atom regex -> sorted uint32 array of the code points it matches under IGNORECASE
_CACHE = {}     # (digest, patterns) -> LogTables


def _all():
    global _ALL
    if _ALL is None:
        _ALL = np.arange(MAXCP, dtype="<u4").tobytes().decode("utf-32-le", "surrogatepass")
    return _ALL


def separators():
    """Code points at which str.splitlines() of this interpreter splits, ascending (cached)."""
    global _SEPS
    if _SEPS is None:
        # chr(13) is followed by chr(14) in _all(), never by "\n": every separator ends its own piece
        _SEPS = [ord(p[-1]) for p in _all().splitlines(True)[:-1]]
    return _SEPS


def _atom_cps(atom):
    cps = _ATOM_CP.get(atom)
    if cps is None:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            hits = re.compile(atom, re.IGNORECASE).findall(_all())
        if any(len(h) != 1 for h in hits[:1000]):
            raise PatternsUnsupported(f"atom {atom!r} does not match exactly one code point")
        cps = np.frombuffer("".join(hits).encode("utf-32-le", "surrogatepass"), dtype="<u4")
        _ATOM_CP[atom] = cps
    return cps


class LogTables:
    """The matcher's tables for one pattern set (field names of csrc/gen_log_dfa.build())."""

    FIELDS = ("nsym", "nstate", "ascii_sym", "ranges", "trans", "out", "SEP", "OTHER", "ncat")

    def __init__(self, patterns, warm, flags=0, **t):
        self.patterns = tuple(patterns)
        self.names = tuple(n for n, _ in self.patterns)
        self.warm = warm
        self.flags = flags  # FLAG_CARRY for a set with loop items
        self.digest = pattern_digest(self.patterns)
        self.unidata = unicodedata.unidata_version
        for k in self.FIELDS:
            setattr(self, k, t[k])
        self._image = {}

    def __getitem__(self, k):  # the dict form gen_log_dfa.simulate walks
        if k not in self.FIELDS:
            raise KeyError(k)
        return getattr(self, k)

    def as_dict(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    @property
    def nrange(self):
        return len(self.ranges)

    def image(self, flags=None):
        """The flat little-endian table image of include/krca.h (krca_log_tables_check).  flags: the
        header's flag word instead of the set's own (tests force FLAG_CARRY on a fixed-length set to
        compare the carried long-line kernel with the speculative one)."""
        flags = self.flags if flags is None else int(flags)
        if flags not in self._image:
            body = bytes(self.ascii_sym) + np.asarray(self.ranges, "<u4").reshape(-1, 3).tobytes() + \
                np.asarray(self.trans, "<u2").tobytes() + np.asarray(self.out, "<u2").tobytes()
            body += b"\0" * (-len(body) % 8)
            head = IMAGE_HEADER.pack(IMAGE_MAGIC, IMAGE_VERSION, self.ncat, self.nsym, self.nstate, self.nrange,
                                     self.warm, self.OTHER, self.digest, IMAGE_HEADER.size + len(body), flags)
            self._image[flags] = head + body
        return self._image[flags]


def _symbol(tables, c):
    if c < 128:
        return tables["ascii_sym"][c]
    ranges = tables["ranges"]
    sym, lo, hi = tables["OTHER"], 0, len(ranges) - 1
    while lo <= hi:
        mid = (lo + hi) >> 1
        if c < ranges[mid][0]:
            hi = mid - 1
        elif c > ranges[mid][1]:
            lo = mid + 1
        else:
            sym = ranges[mid][2]
            break
    return sym


def simulate(tables, line):
    """Python model of the device matcher on one line (no separators inside) -> category mask."""
    st, m = 0, 0
    for ch in line:
        sym = _symbol(tables, ord(ch))
        assert sym != tables["SEP"]
        st = tables["trans"][st][sym]
        m |= tables["out"][st]
    return m


def simulate_segments(tables, line, nseg=64):
    """Python restatement of log_dfa_long_carry_rt (csrc/log_rt.h) on one line -> (mask, rounds).

    The line's UTF-8 bytes are cut into ``nseg`` segments of ceil(bytes / nseg) bytes; lane i owns
    the code points whose first byte lies in segment i.  Each lane warms up from the start state
    over the <= ``warm`` code points before its first one, notes the state it enters its segment
    with (``entry``), walks to ``exit`` and ORs the masks reported on the way.  Then rounds: ``prev``
    is the predecessor lane's exit (the start state for lane 0); when no lane has prev != entry the
    line is done; else every such lane takes prev as its entry and walks its segment again.  An
    empty segment hands its entry on as its exit.  Masks of superseded walks stay ORed in: every
    walk starts from the state some suffix of the text before it leads to, so whatever it reports
    is a match inside the line.  After round r lanes 0..r are final: at most nseg - 1 rounds."""
    trans, out, warm = tables["trans"], tables["out"], tables.warm
    syms = [_symbol(tables, ord(ch)) for ch in line]
    starts, pos = [], 0  # byte offset of each code point
    for ch in line:
        starts.append(pos)
        pos += len(ch.encode("utf-8", "surrogatepass"))
    seg = (pos + nseg - 1) // nseg
    first = [0] * (nseg + 1)  # first[i]: index of the first code point starting at or after byte i * seg
    k = 0
    for i in range(nseg + 1):
        while k < len(starts) and starts[k] < min(pos, i * seg):
            k += 1
        first[i] = k
    mask = 0

    def walk(i, st):
        nonlocal mask
        for sy in syms[first[i]:first[i + 1]]:
            st = trans[st][sy]
            mask |= out[st]
        return st

    entry, exit_ = [0] * nseg, [0] * nseg
    for i in range(nseg):
        st = 0
        if first[i] > 0 and first[i] < first[i + 1]:
            for sy in syms[max(0, first[i] - warm):first[i]]:
                st = trans[st][sy]
        entry[i] = st
        exit_[i] = walk(i, st)
    rounds = 0
    while True:
        prev = [0] + exit_[:-1]
        redo = [i for i in range(nseg) if prev[i] != entry[i]]
        if not redo:
            return mask, rounds
        rounds += 1
        for i in redo:
            entry[i] = prev[i]
            exit_[i] = walk(i, prev[i])


def minimize(trans, outs):
    """Moore partition refinement, then breadth-first renumbering from the start state (0 stays 0):
    the numbering csrc/gen_log_dfa.minimize gives."""
    n, nsym = len(trans), len(trans[0])
    part = list(outs)
    while True:
        keys = {}
        new = [keys.setdefault((part[s],) + tuple(part[t] for t in trans[s]), len(keys)) for s in range(n)]
        if len(keys) == len(set(part)):
            break
        part = new
    rep = {}
    for s in range(n):
        rep.setdefault(part[s], s)
    ids, order, k = {part[0]: 0}, [part[0]], 0
    while k < len(order):
        r = rep[order[k]]
        for a in range(nsym):
            c = part[trans[r][a]]
            if c not in ids:
                ids[c] = len(order)
                order.append(c)
        k += 1
    return ([[ids[part[trans[rep[c]][a]]] for a in range(nsym)] for c in order], [outs[rep[c]] for c in order])


def _limit(what, value, limit):
    if value > limit:
        raise PatternsUnsupported(f"log pattern set has {value} {what}; the device matcher holds at most {limit}")


def compile_patterns(patterns, unbounded=False):
    """Ordered (name, regex) pairs -> LogTables (cached per process by digest).
    unbounded: also accept ``* + {m,} {,}`` on one atom (module docstring); a set that uses none of
    them compiles to the same tables either way."""
    patterns = tuple((str(n), p) for n, p in patterns)
    if not patterns:
        raise PatternsUnsupported("log pattern set is empty")
    _limit("categories", len(patterns), MAX_NCAT)
    pats = [parse(n, p, unbounded) for n, p in patterns]  # (also: every regex is a str)
    key = (pattern_digest(patterns), patterns)  # (a set with loops gets past parse() only under unbounded)
    hit = _CACHE.get(key)
    if hit is not None:
        return hit
    _limit("alternatives after expansion", sum(len(a) for a in pats), MAX_ALTS)
    atoms = sorted({(a if isinstance(a, str) else a[1]) for alts in pats for alt in alts for a in alt})
    # signature of a code point: which atoms match it, as bits of Python ints packed in uint64 words
    nw = (len(atoms) + 63) // 64
    sig = np.zeros((MAXCP, nw), np.uint64)
    for i, a in enumerate(atoms):
        sig[_atom_cps(a), i // 64] |= np.uint64(1 << (i % 64))
    seps = separators()

    # ---- symbols: distinct signatures of ASCII code points, then OTHER, then the rest -----------
    sig_to_sym, ascii_sym = {}, []
    sepset = set(seps)
    for c in range(128):
        if c in sepset:
            ascii_sym.append(SEP)
            continue
        ascii_sym.append(sig_to_sym.setdefault(sig[c].tobytes(), len(sig_to_sym)))
    # OTHER: what the bulk of the non-ASCII code points (unassigned ones among them) look like
    hi = sig[128:]
    hi_seps = np.array([c - 128 for c in seps if c >= 128], np.int64)
    if nw == 1:
        u1, inv, cnt = np.unique(hi[:, 0], return_inverse=True, return_counts=True)
        uniq = u1.reshape(-1, 1)
    else:
        uniq, inv, cnt = np.unique(hi, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    other_row = int(np.argmax(cnt))
    OTHER = sig_to_sym.setdefault(uniq[other_row].tobytes(), len(sig_to_sym))
    special = inv != other_row
    special[hi_seps] = True
    sp = np.flatnonzero(special)
    is_sep = np.isin(sp, hi_seps)
    rows = inv[sp]
    urows, first = np.unique(rows[~is_sep], return_index=True)
    row_sym = np.full(len(uniq), -1, np.int64)
    for r in urows[np.argsort(first)].tolist():  # numbered in code point order of first appearance
        row_sym[r] = sig_to_sym.setdefault(uniq[r].tobytes(), len(sig_to_sym))
    sp_sym = np.where(is_sep, SEP, row_sym[rows])
    cps = sp + 128
    brk = np.flatnonzero((np.diff(cps) != 1) | (np.diff(sp_sym) != 0)) + 1  # first code point of each run
    lo_i = np.concatenate(([0], brk)) if len(cps) else np.zeros(0, np.int64)
    hi_i = np.concatenate((brk - 1, [len(cps) - 1])) if len(cps) else lo_i
    ranges = [[int(cps[a]), int(cps[b]), int(sp_sym[a])] for a, b in zip(lo_i.tolist(), hi_i.tolist())]
    nsym = len(sig_to_sym)
    _limit("symbols (classes of code points the patterns tell apart)", nsym, MAX_NSYM)
    _limit("non-ASCII code point ranges", len(ranges), MAX_NRANGE)
    sym_bits = [None] * nsym  # per symbol: the atoms matching it, as one Python int
    for s, i in sig_to_sym.items():
        sym_bits[i] = int.from_bytes(s, "little")
    atom_bit = {a: 1 << i for i, a in enumerate(atoms)}

    # ---- subset construction over NFA positions (pattern, alt, item) ------------------------------
    # An item is an atom or a loop item.  closure(p, a, i): the position and, past every loop item from
    # it on, the next one.  A loop item that matches the symbol stays (its closure), an atom that matches
    # advances (the next position's closure); a position at the end of its alternative reports the
    # category.  Search semantics: the closure of every alternative's position 0 belongs to every state
    # and is kept out of the state sets.  Positions are numbered and a state is the int of their bits.
    alts = [(p, [(a if isinstance(a, str) else a[1], not isinstance(a, str)) for a in alt])
            for p, al in enumerate(pats) for alt in al]
    base, npos = [], 0
    for _, items in alts:
        base.append(npos)
        npos += len(items) + 1
    closure, end_cat = [0] * npos, [0] * npos
    for (p, items), b in zip(alts, base):
        end_cat[b + len(items)] = 1 << p
        for i in range(len(items), -1, -1):
            closure[b + i] = 1 << (b + i)
            if i < len(items) and items[i][1]:
                closure[b + i] |= closure[b + i + 1]
    always = 0
    for b in base:
        always |= closure[b]
    succ = [[0] * npos for _ in range(nsym)]  # succ[sym][position]: where the symbol takes it
    for (p, items), b in zip(alts, base):
        for i, (atom, loop) in enumerate(items):
            bit = atom_bit[atom]
            for sym in range(nsym):
                if sym_bits[sym] & bit:
                    succ[sym][b + i] = closure[b + i] if loop else closure[b + i + 1]

    def bits(x):
        while x:
            low = x & -x
            yield low.bit_length() - 1
            x ^= low

    always_pos = list(bits(always))
    from_always = [0] * nsym
    for sym in range(nsym):
        for q in always_pos:
            from_always[sym] |= succ[sym][q]

    def out(state):
        m = 0
        for q in bits(state):
            m |= end_cat[q]
        return m

    states, order, trans, k = {0: 0}, [0], [], 0
    while k < len(order):
        row, here = [], list(bits(order[k]))
        for sym in range(nsym):
            nx, sc = from_always[sym], succ[sym]
            for q in here:
                nx |= sc[q]
            nx &= ~always
            if nx not in states:
                states[nx] = len(order)
                order.append(nx)
                _limit("states before minimisation", len(order), 8 * MAX_NSTATE)
            row.append(states[nx])
        trans.append(row)
        k += 1
    trans, outs = minimize(trans, [out(s) for s in order])
    _limit("states", len(trans), MAX_NSTATE)
    loops = any(loop for _, items in alts for _, loop in items)
    if loops:  # loops at their minimum; only the speculation's warm-up
        warm = min(63, max(sum(not loop for _, loop in items) for _, items in alts) - 1)
    else:
        warm = max(len(items) for _, items in alts) - 1
    t = LogTables(patterns, warm, flags=FLAG_CARRY if loops else 0, nsym=nsym, nstate=len(trans),
                  ascii_sym=ascii_sym, ranges=ranges, trans=trans, out=outs, SEP=SEP, OTHER=OTHER, ncat=len(pats))
    _CACHE[key] = t
    return t
