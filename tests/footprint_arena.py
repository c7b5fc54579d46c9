"""TEST HELPER (not a conftest) of tests/test_dev_footprint.py: a guarded ARENA that every device buffer of a case of tests/stream_cases.py is
carved from, and the CHECKER of what a call left in it.  Pure numpy: the arena is laid out and filled on the host as one array of 32-bit
words, the GPU test uploads it as one torch int32 tensor, hands the entry point pointers into it and downloads it whole; the checker compares
the two host arrays and needs no device.

Layout.  Buffers in the order of the case (inputs, then pure outputs), each starting on a 256-byte boundary, a guard band before the first,
between any two and after the last: at least GUARD_ROWS rows x pitch floats next to a "field" buffer (more than the 27-step prologue of the
wave pipeline plus its 16-row read halo), at least GUARD_FLAT floats next to a "flat" one.  Guards hold the quiet-NaN word 0x7FC0ABCD (the
pattern of tests/test_snaps.py): a value pulled in from one is a NaN in the answer.  Fields hold their values in [:, :nze] and +0.0 in the
padding columns [nze, pitch) -- or, where the case names one for the buffer (Case.pad_words: the excitation maps and images, of which
fdwave.h says "padding columns keep their words", not "are zero"), a sentinel word; pure outputs hold the case's sentinel.  A buffer of
kind "ifield" is a field of int32 words (d_texc): the case hands it over as an int32 array and it travels as words from there to the
comparison, never through a float conversion.  Everything a stray access of a few dozen rows could reach is memory of this one allocation.

The four rules (fdwave.h: padding columns are zero and stay zero, `const` arrays are only read, a call on rows [r0, r1) writes only those
rows, the fused fdw_dev_back4 leaves d_lvl0 / d_lvl1 untouched):
  (a) guards      every guard word is bit-identical;
  (b) pads        every padding word of every field buffer equals the upload bit for bit (+0.0, or the buffer's pad word);
  (c) read-only   a buffer that no label names and that is not on the case's scratch list is bit-identical to what was uploaded;
  (d) rows        where a label carries rows (or the case states written_rows for the buffer), the rows outside hold what was uploaded --
                  damped once where the case itself hands the buffer to fdw_dev_taper_finalize after the call (case.finalized): that pass
                  is the case's own, it covers every row, and the checker is given its CPU restatement.
A violation names the rule, the case, the buffer, row and column, and for a guard word the offset to the nearest buffer."""
import numpy as np

GUARD_WORD = 0x7FC0ABCD
GUARD_ROWS = 48
GUARD_FLAT = 1024
ALIGN = 64                  # words: 256 bytes
FIELD_KINDS = ("field", "ifield")      # [rows][pitch] on the device; "ifield": int32 words
MAX_REPORTED = 6            # violations listed per rule and buffer


def pitch_of(nze):
    """fdw_pitch of a context with nze columns (rows are 256-byte aligned); the GPU test asserts that the context agrees."""
    return (nze + 63) // 64 * 64


class Buf:
    """One buffer of the arena: words [off, off + rows * cols); a field has cols = pitch and nze value columns, a flat buffer is dense."""

    def __init__(self, name, kind, off, shape, nze, pitch):
        self.name, self.kind, self.off = name, kind, off
        if kind in FIELD_KINDS:
            self.rows, self.cols, self.nze = shape[0], pitch, nze
            assert shape[1] == nze, (name, shape, nze)
        else:
            self.rows, self.cols = (int(np.prod(shape[:-1])), shape[-1]) if len(shape) > 1 else (1, shape[0])
            self.nze = self.cols
        self.shape = tuple(shape)
        self.size = self.rows * self.cols

    def view(self, words):
        """The buffer's words in an arena array, as [rows][cols]."""
        return words[self.off:self.off + self.size].reshape(self.rows, self.cols)

    def values(self, words):
        """What a test compares: float32 [rows][nze] of a field (of an "ifield": its int32 words seen as float32, as the answers of
        tests/stream_cases.py carry them), the dense array of a flat buffer (in the case's shape)."""
        a = self.view(words).view(np.float32)
        return np.ascontiguousarray(a[:, :self.nze]) if self.kind in FIELD_KINDS else np.ascontiguousarray(a).reshape(self.shape)


class Arena:
    """The layout of one case and its uploaded image `up` (uint32).  bufs: {name: Buf} in arena order; guard: bool mask of the guard words."""

    def __init__(self, case, nze, contents, damp=None):
        """contents: [(name, kind, float32 array)] in arena order, fields dense [nxl][nze] (an "ifield": the float32 VIEW of its int32 words, see
        words_of); damp(dense field) -> the field after one pass of fdw_dev_taper_finalize (needed where the case finalizes a buffer on which
        rule (d) looks at rows)."""
        self.case, self.nze, self.pitch = case, nze, pitch_of(nze)
        pad_words = getattr(case, "pad_words", {})
        need = [GUARD_ROWS * self.pitch if kind in FIELD_KINDS else GUARD_FLAT for _, kind, _ in contents]
        self.bufs, off = {}, 0
        for k, (name, kind, arr) in enumerate(contents):
            gap = max(need[k], need[k - 1] if k else 0)
            off = -(-(off + gap) // ALIGN) * ALIGN
            b = Buf(name, kind, off, arr.shape, nze, self.pitch)
            self.bufs[name] = b
            off += b.size
        self.size = -(-(off + need[-1]) // ALIGN) * ALIGN
        self.up = np.full(self.size, GUARD_WORD, np.uint32)
        self.guard = np.ones(self.size, bool)
        for name, kind, arr in contents:
            b = self.bufs[name]
            self.guard[b.off:b.off + b.size] = False
            v = b.view(self.up)
            v[:] = pad_words.get(name, 0) if kind in FIELD_KINDS else 0      # the padding columns: +0.0, or the case's word for the buffer
            assert arr.dtype == np.float32, (name, arr.dtype)              # (so that the next line copies words and converts nothing)
            v[:, :b.nze] = np.ascontiguousarray(arr).reshape(b.rows, b.nze).view(np.uint32)
        self.up.setflags(write=False)
        self.outside = {}      # {buffer: uint32 [rows][nze]} what rule (d) expects outside the written rows where that is not the upload
        for name, kind, arr in contents:
            if name in case.finalized:
                self.outside[name] = np.ascontiguousarray(damp(np.array(arr, np.float32, order="C")), np.float32).view(np.uint32)

    def pointers(self, base):
        """{buffer: device address} for an arena uploaded at address `base`."""
        assert base % (4 * ALIGN) == 0, f"the arena itself is not 256-byte aligned: {base:#x}"
        return {name: base + 4 * b.off for name, b in self.bufs.items()}

    def where(self, w):
        """Word offset w in words: inside a buffer, or in a guard relative to the nearest buffer."""
        for b in self.bufs.values():
            if b.off <= w < b.off + b.size:
                r, c = divmod(w - b.off, b.cols)
                return f"{b.name}[{r}][{c}]" + (" (a padding column)" if c >= b.nze else "")
        best = None
        for b in self.bufs.values():
            d = w - b.off if w < b.off else w - (b.off + b.size) + 1
            if best is None or abs(d) < abs(best[1]):
                best = (b, d)
        b, d = best
        if d < 0:
            r, c = divmod(-d, b.cols)
            return f"guard, {-d} floats BEFORE {b.name} ({r} rows and {c} floats of its pitch {b.cols})"
        r, c = divmod(d - 1, b.cols)
        return f"guard, {d} floats AFTER the end of {b.name} (row {b.rows + r}, column {c} if it went on)"


def words_of(kind, arr):
    """What a case hands over for a buffer, as the float32 array the arena copies word for word: an "ifield" must BE int32 and is only viewed."""
    if kind == "ifield":
        arr = np.ascontiguousarray(arr)
        assert arr.dtype == np.int32, arr.dtype
        return arr.view(np.float32)
    return np.asarray(arr, np.float32)


def build(case, inputs, damp=None):
    """The arena of a case for the argument set `inputs` (stream_cases.inputs(deck, v)); damp: see Arena."""
    nze = inputs["d"]["nze"]
    contents = [(name, kind, words_of(kind, arr)) for name, (kind, arr) in case.ins(inputs).items()]
    contents += [(name, kind, np.full(shape, val, np.float32)) for name, (kind, shape, val) in case.outs.items()]
    return Arena(case, nze, contents, damp)


def _rows_mask(rows, n):
    m = np.zeros(n, bool)
    m[rows] = True
    return m


def written_rows(arena, labels):
    """{buffer: bool mask of the rows the call may write} for the buffers on which rule (d) has something to say: the case's written_rows,
    else the rows of the buffer's labels (only where every label of the buffer carries rows and is compared as it lies, without a post)."""
    out = {}
    for label, name, post, rows in labels:
        if name in arena.case.written_rows:
            continue
        n = arena.bufs[name].rows
        m = np.ones(n, bool) if rows is None or post is not None else _rows_mask(rows, n)
        out[name] = out.get(name, np.zeros(n, bool)) | m
    for name, rows in arena.case.written_rows.items():
        out[name] = _rows_mask(rows, arena.bufs[name].rows)
    return {name: m for name, m in out.items() if not m.all()}


def check(arena, down, labels, rules="abcd"):
    """The violations (strings) of rules (a) to (d) in the downloaded arena `down` (uint32, the arena's size); [] if there is none."""
    up, case = arena.up, arena.case
    down = np.asarray(down).view(np.uint32).ravel()
    assert down.shape == up.shape
    out = []

    def report(rule, what, words):
        for w in words[:MAX_REPORTED]:
            out.append(f"{case.name}: rule ({rule}) {what}: {arena.where(int(w))}, arena word {int(w)}: {int(up[w]):#010x} -> {int(down[w]):#010x}")
        if len(words) > MAX_REPORTED:
            out.append(f"{case.name}: rule ({rule}) {what}: ... {len(words)} words in all, the last at {arena.where(int(words[-1]))}")

    if "a" in rules:
        report("a", "a guard word changed", np.flatnonzero(arena.guard & (down != up)))
    named = {name for _, name, _, _ in labels}
    may_write = written_rows(arena, labels)
    for b in arena.bufs.values():
        idx = np.arange(b.off, b.off + b.size).reshape(b.rows, b.cols)
        changed = b.view(down) != b.view(up)
        if "b" in rules and b.kind in FIELD_KINDS:
            pad = int(getattr(case, "pad_words", {}).get(b.name, 0))
            assert (b.view(up)[:, b.nze:] == pad).all()
            report("b", f"a padding column of {b.name} does not hold its word {pad:#010x}" if pad else f"a padding column of {b.name} is not +0.0",
                   idx[:, b.nze:][changed[:, b.nze:]])
        if "c" in rules and b.name not in named and b.name not in case.scratch:
            report("c", f"{b.name} is only read by this call (or left untouched) and changed", idx[:, :b.nze][changed[:, :b.nze]])
        if "d" in rules and b.name in may_write:
            keep = ~may_write[b.name]
            moved = b.view(down)[:, :b.nze] != arena.outside[b.name] if b.name in arena.outside else changed[:, :b.nze]
            report("d", f"a row of {b.name} outside the rows asked for changed", idx[keep, :b.nze][moved[keep]])
    return out


def results(arena, down, labels):
    """{label: host array} of what the call left, cut out of the downloaded arena as stream_cases.Run.results cuts it out of its tensors."""
    down = np.asarray(down).view(np.uint32).ravel()
    out = {}
    for label, name, post, rows in labels:
        a = arena.bufs[name].values(down)
        if post is not None:
            a = post(a)
        out[label] = a if rows is None else a[rows]
    return out
