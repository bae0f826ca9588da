"""Guard bands for kernel tests: outputs as views into a sentinel-filled buffer, inputs as views into a NaN-filled one.

guarded()  -> an output (or accumulate target) of row stride `ld` between two bands of >= 128 rows; Guard.check() proves that nothing but the view was
              written and, for outputs, that every element of the view was.
poisoned() -> a copy of an input whose row padding and neighbouring rows are NaN: a correct kernel's valid results do not depend on them.

The sentinel is one fixed bit pattern per element width, a quiet NaN in float32 and in bfloat16, and it is compared as integers - a float compare could
not tell it from any other NaN, and could not see it at all in an integer buffer.  The poison of the inputs is ANOTHER NaN pattern: arithmetic hands a NaN
operand's payload on, so a stray store of `x + poison` would otherwise write the very bits the guard expects to find there."""
import torch

BAND_ROWS = 128                      # a stray store of a whole 128-row tile still lands inside the allocation
ALIGN = 16                           # bytes: the view's base address
SENTINEL = {1: 0xA5, 2: 0x7FE5, 4: 0x7FE5C3A7, 8: 0x7FE5C3A75AD2B4E1}          # by element size; 2 / 4: quiet NaNs of bfloat16 / float32
#                                      1: the uint8 outputs hold 0 or 1 (is_endpoint) or flag bits 0..2 (stage_flags), never 0xA5
POISON = {2: 0x7FD3, 4: 0x7FD3A1B7}           # inputs: quiet NaNs too, but not the sentinel's bits (nor its bf16 rounding)
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _backing(n_elems, es, device, pattern=SENTINEL):
    """flat integer buffer of n_elems + slack elements full of the pattern, and the element offset at which a 16-byte aligned address lies"""
    slack = 2 * (ALIGN // es)          # one group to align the buffer's base, one to align the view's
    buf = torch.full((n_elems + slack,), pattern[es], dtype=_INT[es], device=device)
    mis = buf.data_ptr() % ALIGN
    assert mis % es == 0
    return buf, ((ALIGN - mis) % ALIGN) // es


class Guard:
    """handle of a guarded() view: the integer image of the whole backing buffer, where the view lies in it, and what it held when it was armed"""

    def __init__(self, bits, view, off, rows, cols, ld, is_output):
        self.bits, self.view, self.off, self.rows, self.cols, self.ld, self.is_output = bits, view, off, rows, cols, ld, is_output
        self.front_rows = off // ld
        self.back_rows = (bits.numel() - off - rows * ld) // ld
        self.rearm()

    def rearm(self):
        """take what the buffer holds now as the state every element outside the valid region must keep (call after presetting parts of the view by hand)"""
        self._snap = self.bits.cpu().clone()

    def _where(self, flat_index):
        rel = int(flat_index) - self.off
        return rel // self.ld, rel % self.ld            # floor division: rows of the front band are negative

    def check(self, valid=None, written=None):
        """valid: bool [rows, cols], the elements of the view the kernel owns (default: all of them); everything else - bands, row padding, the other elements
        of the view - must hold what it held when armed.  written (default: True for outputs, False where fill= preset the view): no valid element may
        still hold the sentinel."""
        now = self.bits.cpu()
        own = torch.zeros(now.numel(), dtype=torch.bool)
        inside = torch.as_strided(own, (self.rows, self.cols), (self.ld, 1), self.off)
        if valid is None:
            inside.fill_(True)
        else:
            assert tuple(valid.shape) == (self.rows, self.cols)
            inside.copy_(valid.cpu())
        stray = (now != self._snap) & ~own
        if bool(stray.any()):
            r, c = self._where(torch.nonzero(stray)[0, 0])
            raise AssertionError(f"stray write outside the view at (row {r}, column {c}) of a [{self.rows}, {self.cols}] view with row stride {self.ld}; "
                                 f"{int(stray.sum())} elements changed")
        if self.is_output if written is None else written:
            left = (now == SENTINEL[now.element_size()]) & own
            if bool(left.any()):
                r, c = self._where(torch.nonzero(left)[0, 0])
                raise AssertionError(f"element (row {r}, column {c}) of the [{self.rows}, {self.cols}] view was never written; {int(left.sum())} elements left")


def guarded(rows, cols, dtype, ld=None, device="cpu", fill=None):
    """-> (view [rows, cols] of row stride ld, Guard).  The view's base is 16-byte aligned and BAND_ROWS * ld sentinel elements (at least) lie in front of
    it and behind its last row; fill (a number or a [rows, cols] tensor) presets the view: accumulate targets and inputs."""
    ld = cols if ld is None else ld
    assert ld >= cols and rows > 0
    es = torch.empty((), dtype=dtype).element_size()
    band = BAND_ROWS * ld
    bits, a0 = _backing(band + rows * ld + band, es, device)
    off = a0 + band + (-band * es % ALIGN) // es     # the base of the view itself, not of the buffer, is what the kernels' vector stores see
    typed = bits if dtype in _INT.values() else bits.view(dtype)
    view = torch.as_strided(typed, (rows, cols), (ld, 1), off)
    assert view.data_ptr() % ALIGN == 0
    if fill is not None:
        if torch.is_tensor(fill):
            view.copy_(fill.to(device=device, dtype=dtype))
        else:
            view.fill_(fill)
    return view, Guard(bits, view, off, rows, cols, ld, is_output=fill is None)


def guarded_set(spec, device):
    """spec: name -> (rows, cols, dtype).  -> (name -> view, name -> Guard): the out= dict of a binding that takes the caller's outputs, and its guards"""
    pairs = {k: guarded(rows, cols, dtype, device=device) for k, (rows, cols, dtype) in spec.items()}
    return {k: p[0] for k, p in pairs.items()}, {k: p[1] for k, p in pairs.items()}


def guarded_run(fn, unwritten=(), untouched=()):
    """fn(out=None) -> dict of output tensors, a *_device binding.  One run for the shapes, a second one with every output a guarded view of that dtype and
    size, then every guard is checked: written, but for the names in `unwritten` (may keep sentinels; True / False: all / none of them) and `untouched` (must keep them all).
    -> the second dict"""
    first = fn()
    views, guards = guarded_set({k: (t.shape[0], t[0].numel(), t.dtype) for k, t in first.items()}, next(iter(first.values())).device)
    out = fn(out=views)
    assert sorted(out) == sorted(views) and all(out[k].data_ptr() == views[k].data_ptr() for k in views)
    for k, g in guards.items():
        g.check(valid=torch.zeros(g.rows, g.cols, dtype=torch.bool) if k in untouched else None, written=k not in unwritten if isinstance(unwritten, tuple) else not unwritten)
    return out


def poisoned(t, ld=None, extra_rows=0, front_rows=0, device=None):
    """a copy of the 2-D tensor t as a [rows, cols] view of row stride ld (default cols + one 16-byte group) into a NaN-filled buffer: NaN row padding,
    extra_rows NaN rows behind the last row and front_rows in front of the first; base 16-byte aligned.  Never for what a library defines as zero."""
    rows, cols = t.shape
    es = t.element_size()
    ld = cols + ALIGN // es if ld is None else ld
    assert ld >= cols and t.dtype in (torch.float32, torch.bfloat16)
    device = t.device if device is None else device
    bits, a0 = _backing((front_rows + rows + extra_rows) * ld, es, device, POISON)
    off = a0 + front_rows * ld + (-front_rows * ld * es % ALIGN) // es
    view = torch.as_strided(bits.view(t.dtype), (rows, cols), (ld, 1), off)
    view.copy_(t.to(device))
    return view
