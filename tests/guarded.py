"""A device output buffer between two guard bands, for the tests that call the C ABI with raw pointers (tests/test_gpu_depth.py,
tests/test_gpu_envmap_edges.py): every element the kernel must write is written, nothing around the output is."""
import torch

GUARD = 4096


class Guarded:
    """[GUARD | n | GUARD] elements of ``dtype`` filled with a NaN (or 0xAB) pattern; ``ptr``: the address of the middle slice."""
    PATTERN = {torch.float32: (torch.int32, 0x7FC00ABC), torch.float64: (torch.int64, 0x7FF8000000000ABC), torch.uint8: (torch.uint8, 0xAB)}

    def __init__(self, n, dev, dtype=torch.float32):
        self.n, self.dtype = n, dtype
        self.itype, self.pat = self.PATTERN[dtype]
        self.bits = torch.full((n + 2 * GUARD,), self.pat, dtype=self.itype, device=dev)
        self.ptr = self.bits[GUARD:].data_ptr()

    def body(self):
        return self.bits[GUARD:GUARD + self.n].view(self.dtype)

    def check(self, what, all_written=True):
        if all_written:
            unwritten = int((self.bits[GUARD:GUARD + self.n] == self.pat).sum())
            assert unwritten == 0, "%s: %d of %d elements were never written" % (what, unwritten, self.n)
        for side, guard in (("below", self.bits[:GUARD]), ("above", self.bits[GUARD + self.n:])):
            touched = (guard != self.pat).nonzero().flatten()
            assert touched.numel() == 0, "%s: %d elements %s the output were written (first at guard offset %d)" % (
                what, touched.numel(), side, int(touched[0]))
        return self.body()
