"""Plain-Python model of the entropy phase of sais_amd/csrc/jpeg.hip (tests only): the destuffed layout of jpeg_destuff, locate(),
run() on the state (bit position, slot, k), jpeg_sync_spec with its warm-up, and jpeg_sync_pass as Jacobi iteration (every
subsequence of pass p reads the exits of pass p - 1).  model(file) says how many passes the file needs; the tests derive from that
which status the GPU must report.

The kernel iterates asynchronously: a thread may read its predecessor's exit of this pass or of the last one.  Two bounds follow.
  - Every state the kernel holds after pass t is a Jacobi state of some time >= t, so it settles no later than the model:
    P <= MAX_PASSES - 2 means the flag of the last pass stays clear and the status is 0.
  - The lanes of one wave load their predecessors' exits in one instruction, so inside a wave the correct prefix grows by one
    subsequence per pass, and by one more where the predecessor sits in a wave that ran earlier in the same launch: at most 2 per
    pass.  The kernel therefore needs at least P / 2 passes; MUST_FAIL_P = 8 * MAX_PASSES leaves a factor of 4 over that bound.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref  # noqa: E402

SUB_BYTES, WARMUP, MAX_PASSES = 128, 6, 32
SUB_BITS = 8 * SUB_BYTES
MUST_DECODE_P = MAX_PASSES - 2            # P <= 30: flags[31] stays 0, the status must be 0
MUST_FAIL_P = 8 * MAX_PASSES              # P >= 256: SAIS_JPEG_E_SYNC must be set (factor 8 over the pass bound, 4 over P / 2)
E_SYNC = 16


def _table(counts, vals):
    """Canonical codes -> {(length, code): symbol} and a list over the 16-bit prefix: (length, symbol), (0, 0) where no code fits."""
    lut, code, k = [(0, 0)] * 65536, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            lo = code << (16 - ln)
            lut[lo:lo + (1 << (16 - ln))] = [(ln, vals[k])] * (1 << (16 - ln))
            code += 1
            k += 1
        code <<= 1
    return lut


class Layout:
    """jpeg_destuff for one image: the scan without stuffed zeros and fill bytes, restart segment s at sego[s] =
    roundup(k0 + 2 s SUB_BYTES), ending at sege[s]; zeros elsewhere."""

    def __init__(self, data):
        hd = jpeg_ref.parse(data)
        self.hd = hd
        hs, vs = hd['comps'][0][1], hd['comps'][0][2]
        self.ny, self.bpm = hs * vs, hs * vs + 2
        self.mcus = -(-hd['w'] // (8 * hs)) * -(-hd['h'] // (8 * vs))
        self.ri = hd['ri']
        self.nseg = -(-self.mcus // self.ri) if self.ri else 1
        d, i, segs, cur = data, hd['scan'], [], bytearray()
        while i < len(d):
            c = d[i]
            if c != 0xFF:
                cur.append(c)
                i += 1
                continue
            nx = d[i + 1] if i + 1 < len(d) else 0
            if nx == 0x00:
                cur.append(0xFF)
                i += 2
            elif nx == 0xFF:
                i += 1                                                 # fill byte
            elif 0xD0 <= nx <= 0xD7:
                segs.append(bytes(cur))
                cur = bytearray()
                i += 2
            else:
                break                                                  # the marker that ends the scan
        segs.append(bytes(cur))
        assert len(segs) == self.nseg, (len(segs), self.nseg)
        scan_bytes = len(data) - hd['scan']
        self.cap = (scan_bytes + 2 * SUB_BYTES * self.nseg + 2 * SUB_BYTES + SUB_BYTES - 1) // SUB_BYTES * SUB_BYTES
        self.nsub = self.cap // SUB_BYTES
        self.sego, self.sege, k0 = [], [], 0
        buf = bytearray(self.cap + 16)
        for s, seg in enumerate(segs):
            o = (k0 + 2 * s * SUB_BYTES + SUB_BYTES - 1) // SUB_BYTES * SUB_BYTES
            self.sego.append(o)
            self.sege.append(o + len(seg))
            buf[o:o + len(seg)] = seg
            k0 += len(seg)
        self.buf = bytes(buf)
        self.dc = [_table(*hd['ht'][(0, s[1])]) for s in hd['sel']]
        self.ac = [_table(*hd['ht'][(1, s[2])]) for s in hd['sel']]
        self._memo = {}

    def locate(self, j):
        """(live, first, last, segment) of subsequence j, as locate() of the kernels."""
        jb = j * SUB_BYTES
        a = -1
        for s in range(self.nseg):
            if self.sego[s] <= jb:
                a = s
        if a < 0 or jb >= self.sege[a]:
            return False, False, False, a
        return True, jb == self.sego[a], jb + SUB_BYTES >= self.sege[a], a

    def peek16(self, pos):
        i = pos >> 3
        return (int.from_bytes(self.buf[i:i + 3], 'big') >> (8 - (pos & 7))) & 0xFFFF if i + 3 <= len(self.buf) else 0

    def run(self, pos, c, k, stop):
        """run<false>() of the kernels: decode codewords from (pos, c, k) while pos < stop -> (pos, c, k, blocks started)."""
        key = (pos, c, k, stop)
        if key in self._memo:
            return self._memo[key]
        count, it = 0, 0
        while it < SUB_BITS + 64 and pos < stop:
            it += 1
            comp = 0 if c < self.ny else c - self.ny + 1
            ln, sym = (self.dc if k == 0 else self.ac)[comp][self.peek16(pos)]
            if ln == 0:
                ln, sym = 16, 0                                        # no code of any length: E_CODE in the write pass
            s, r = (sym, 0) if k == 0 else (sym & 15, sym >> 4)
            if s > (11 if k == 0 else 10):
                s = 0
            pos += ln + s
            if k == 0:
                count += 1
                k = 1
            elif s:
                k = min(k + r, 63) + 1
            elif r == 15:
                k = min(k + 16, 64)
            else:
                k = 64
            if k >= 64:
                k, c = 0, (c + 1) % self.bpm
        self._memo[key] = (pos, c, k, count)
        return self._memo[key]


def spec(L):
    """jpeg_sync_spec: entry and exit of every live subsequence from a guess made WARMUP subsequences earlier."""
    en, ex = {}, {}
    for j in range(L.nsub):
        live, first, last, a = L.locate(j)
        if not live:
            continue
        pos, c, k = L.sego[a] * 8, 0, 0
        if not first:
            if j * SUB_BYTES - WARMUP * SUB_BYTES > L.sego[a]:
                pos = j * SUB_BITS - WARMUP * SUB_BITS
            b = pos + SUB_BITS
            while b <= j * SUB_BITS:
                pos, c, k, _ = L.run(pos, c, k, b)
                b += SUB_BITS
        en[j] = (pos, c, k)
        if not last:
            ex[j] = L.run(pos, c, k, (j + 1) * SUB_BITS)
    return en, ex


def sequential(L):
    """Entry state of every live subsequence by one sequential decode per segment, codeword by codeword."""
    en = {}
    for s in range(L.nseg):
        pos, c, k = L.sego[s] * 8, 0, 0
        j = L.sego[s] // SUB_BYTES
        while j * SUB_BYTES < L.sege[s]:
            while pos < j * SUB_BITS:
                pos, c, k, _ = L.run(pos, c, k, pos + 1)               # one codeword
            en[j] = (pos, c, k)
            j += 1
    return en


def model(data, max_passes=100000):
    """-> dict(subsequences, wrong_guesses, passes (P: the last pass that re-decoded a subsequence, 0 if none), entries)."""
    L = Layout(data)
    en, ex = spec(L)
    guess = dict(en)
    info = {j: L.locate(j) for j in en}
    P = 0
    for p in range(1, max_passes):
        new_en, new_ex, flag = dict(en), dict(ex), False
        for j, (live, first, last, a) in info.items():
            if first:
                continue
            entry = ex[j - 1][:3]
            if entry == en[j]:
                continue
            new_en[j] = entry
            if last:
                continue
            new_ex[j] = L.run(*entry, (j + 1) * SUB_BITS)
            flag = True
        en, ex = new_en, new_ex
        if not flag:
            break
        P = p
    return dict(subsequences=len(en), wrong_guesses=sum(guess[j] != en[j] for j in en), passes=P, entries=en, layout=L)


def expected_status(P):
    """0: the GPU must decode the file; E_SYNC: it must give it up; None: either (only the image is checked)."""
    return 0 if P <= MUST_DECODE_P else E_SYNC if P >= MUST_FAIL_P else None
