"""Lock-step model of the compacted delta stream in half-line units (stream_bits_f32_compact<NT, 16> in csrc/hsad_env.hip): one wave
of 64 lanes, the scan that lists the changed half lines in place in `old` as 16-bit entries, and the store loop over the list.  As in
tests/delta_compact_ref.py every instruction of the wave is modelled as the hardware runs it: all lanes read, then all lanes write.
`old` is held as half-words, the way the 16-bit LDS stores see it; a read of word w puts half-words 2w and 2w + 1 together.

    n        floats of the workgroup's range; nch = n // 4 chunks; a word owns 8 chunks (a 128-byte line), a half word 4 (64 bytes)
    bits     the current bit words, old the words the range was last written from: at least ceil(nch / 8) of each"""

WAVE = 64
SCAN_STEPS = 4      # kScanSteps
STORE_GROUPS = 4    # kStoreGroups


def changed_halves(bits, old, n):
    """the half-line indices (2w, 2w + 1) of the full words whose 16 bits differ, in order"""
    nfull = (n // 4) // 8
    out = []
    for w in range(nfull):
        x = bits[w] ^ old[w]
        if x & 0xffff:
            out.append(2 * w)
        if x >> 16:
            out.append(2 * w + 1)
    return out


def compact16(bits, old, n, scan_steps=SCAN_STEPS, store_groups=STORE_GROUPS):
    """returns (stored (chunk, nibble) pairs in store order, lines counted, units counted, reads of old as (word, value seen),
    list entries, store instructions as lists of (lane, chunk))"""
    mem = []                             # `old` itself, as half-words: the list is written in place
    for v in old:
        mem += [v & 0xffff, v >> 16]
    word = lambda w: mem[2 * w] | (mem[2 * w + 1] << 16)
    nch = n // 4
    nfull = nch // 8
    stored, old_reads, instrs = [], [], []
    count = lines = 0
    for w0 in range(0, nfull, WAVE * scan_steps):
        b, o = [], []
        for u in range(scan_steps):      # the reads of all steps of this trip, every lane, clamped like the kernel's
            ws = [min(w0 + WAVE * u + lane, nfull - 1) for lane in range(WAVE)]
            b.append([bits[w] for w in ws])
            o.append([word(w) for w in ws])
            old_reads += [(w, word(w)) for w in ws]
        for u in range(scan_steps):
            ws = [w0 + WAVE * u + lane for lane in range(WAVE)]
            x = [(b[u][lane] ^ o[u][lane]) if ws[lane] < nfull else 0 for lane in range(WAVE)]
            lo = [(v & 0xffff) != 0 for v in x]
            hi = [(v >> 16) != 0 for v in x]
            rank, below = [], 0                                                   # mbcnt(m_lo) + mbcnt(m_hi)
            for lane in range(WAVE):
                rank.append(below)
                below += lo[lane] + hi[lane]
            for lane in range(WAVE):                                              # the store of the lo entries, then of the hi ones
                if lo[lane]:
                    pos = count + rank[lane]
                    assert pos <= 2 * ws[lane], "lo entry beyond the word its lane read"
                    mem[pos] = 2 * ws[lane]
            for lane in range(WAVE):
                if hi[lane]:
                    pos = count + rank[lane] + (1 if lo[lane] else 0)
                    assert pos <= 2 * ws[lane] + 1, "hi entry beyond the word its lane read"
                    mem[pos] = 2 * ws[lane] + 1
            count += sum(lo) + sum(hi)                                            # popc(m_lo) + popc(m_hi)
            lines += sum(1 for a, c in zip(lo, hi) if a or c)                     # popc(m_lo | m_hi)
    # the partial last word: lanes 0 .. (nch & 7) - 1, whole word, direct form
    part = []
    for lane in range(WAVE):
        kp = 8 * nfull + lane
        if kp < nch:
            old_reads.append((nfull, word(nfull)))
            if bits[nfull] != word(nfull):
                part.append((kp, (bits[nfull] >> (4 * (lane & 7))) & 15))
    entries = mem[:count]

    def group(e0, u, masked):
        ins = []
        for lane in range(WAVE):
            e = e0 + 16 * u + (lane >> 2)
            h = mem[min(e, count - 1)]
            c = lane & 3
            if not masked or e < count:
                k = 4 * h + c
                stored.append((k, (bits[h >> 1] >> (16 * (h & 1) + 4 * c)) & 15))
                ins.append((lane, k))
        instrs.append(ins)

    e0 = 0
    while e0 + 16 * store_groups <= count:                                        # full blocks: no lane is off
        for u in range(store_groups):
            group(e0, u, False)
        e0 += 16 * store_groups
    if e0 < count:
        for u in range(store_groups):
            group(e0, u, True)
    stored += part
    part_units = 1 if (nch & 7) <= 4 else 2
    return stored, lines + (1 if part else 0), count + (part_units if part else 0), old_reads, entries, instrs
