"""Sentinel-guarded device views for the kernel-level parity modules -- TEST INFRASTRUCTURE ONLY.

A Region is a [M, width] fp32 view with row pitch `pitch` and column offset `off` inside a sentinel-filled device buffer: a kernel
that writes past a row, before the first row or after the last one changes a sentinel, and get() / untouched() see it."""
import torch

BAND = 256
SENT = 1.3e36


class Region:
    """A [M, width] fp32 view with row pitch `pitch` and column offset `off` inside a sentinel-filled device buffer."""

    def __init__(self, M, width, pitch=None, off=0, fill=None):
        self.M, self.width, self.off = M, width, off
        self.pitch = pitch if pitch is not None else width + off + 4
        assert self.pitch >= off + width
        self.buf = torch.full((2 * BAND + M * self.pitch,), SENT, dtype=torch.float32, device="cuda")
        self.v = self.buf[BAND:BAND + M * self.pitch].view(M, self.pitch)[:, off:off + width]
        if fill is not None:
            self.v.copy_(fill.float())

    def get(self, what=""):
        """The view's content (CPU, fp64) after checking that nothing outside it was written."""
        torch.cuda.synchronize()
        rest = self.buf.clone()
        rest[BAND:BAND + self.M * self.pitch].view(self.M, self.pitch)[:, self.off:self.off + self.width] = SENT
        assert bool((rest == SENT).all()), "guard band overwritten: " + what
        return self.v.cpu().double()

    def bits(self, what=""):
        """The view's content as fp32 on the CPU (for bitwise comparisons), guard bands checked."""
        self.get(what)
        return self.v.cpu().clone()

    def untouched(self):
        """True if the whole buffer, the view included, still holds the sentinel (an output no call has written)."""
        torch.cuda.synchronize()
        return bool((self.buf == SENT).all())

    @property
    def ptr(self):
        return self.v.data_ptr()
