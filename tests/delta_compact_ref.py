"""Lock-step model of the compacted delta stream of the pipelined rollout (stream_bits_f32_compact in csrc/hsad_env.hip): one wave of
64 lanes, the scan that lists the changed words in place in `old`, and the store loop over the list.  Every instruction of the wave is
modelled as the hardware runs it: all lanes read, then all lanes write.  The model records each read of `old` with the value it saw
and each float4 chunk it stores, so a test can hold it to the direct form (stream_bits_f32_delta) and to the in-place invariant.

    n        floats of the workgroup's range (ng * P * F); nch = n // 4 chunks, a word owns 8 chunks (one 128-byte line)
    bits     the current bit words, old the words the range was last written from: at least ceil(nch / 8) of each"""

WAVE = 64
SCAN_STEPS = 4      # kScanSteps: scan steps whose reads are issued together, ahead of their writes
STORE_GROUPS = 4    # kStoreGroups


def direct(bits, old, n):
    """stream_bits_f32_delta without `all`: the (chunk, nibble) pairs stored and the number of lines counted"""
    nch = n // 4
    stored, lines = [], 0
    for k in range(nch):
        w = bits[k >> 3]
        if w != old[k >> 3]:
            stored.append((k, (w >> (4 * (k & 7))) & 15))
            lines += (k & 7) == 0
    return stored, lines


def compact(bits, old, n, scan_steps=SCAN_STEPS, store_groups=STORE_GROUPS):
    """returns (stored pairs in store order, lines counted, reads of old as (position, value seen), list entries)"""
    lst = list(old)                      # `old` itself: the list is written in place
    nch = n // 4
    nfull = nch // 8
    stored, old_reads = [], []
    count = 0
    for w0 in range(0, nfull, WAVE * scan_steps):
        b, o = [], []
        for u in range(scan_steps):      # the reads of all steps of this trip, every lane, clamped like the kernel's
            ws = [min(w0 + WAVE * u + lane, nfull - 1) for lane in range(WAVE)]
            b.append([bits[w] for w in ws])
            o.append([lst[w] for w in ws])
            old_reads += [(w, lst[w]) for w in ws]
        for u in range(scan_steps):
            ws = [w0 + WAVE * u + lane for lane in range(WAVE)]
            changed = [ws[lane] < nfull and b[u][lane] != o[u][lane] for lane in range(WAVE)]
            rank = [sum(changed[:lane]) for lane in range(WAVE)]          # mbcnt of the ballot
            for lane in range(WAVE):
                if changed[lane]:
                    assert count + rank[lane] <= ws[lane], "entry position beyond the word it names"
                    lst[count + rank[lane]] = ws[lane]
            count += sum(changed)                                          # popcount of the ballot
    # the partial last word: lanes 0 .. (nch & 7) - 1, direct form
    part = []
    for lane in range(WAVE):
        kp = 8 * nfull + lane
        if kp < nch:
            old_reads.append((nfull, lst[nfull]))
            if bits[nfull] != lst[nfull]:
                part.append((kp, (bits[nfull] >> (4 * (lane & 7))) & 15))
    entries = lst[:count]
    e0 = 0
    while e0 + 8 * store_groups <= count:                                  # full blocks: no lane is off
        for u in range(store_groups):
            for lane in range(WAVE):
                idx = lst[e0 + 8 * u + (lane >> 3)]
                stored.append((8 * idx + (lane & 7), (bits[idx] >> (4 * (lane & 7))) & 15))
        e0 += 8 * store_groups
    if e0 < count:
        for u in range(store_groups):
            for lane in range(WAVE):
                e = e0 + 8 * u + (lane >> 3)
                idx = lst[min(e, count - 1)]
                if e < count:
                    stored.append((8 * idx + (lane & 7), (bits[idx] >> (4 * (lane & 7))) & 15))
    stored += part
    return stored, count + (1 if part else 0), old_reads, entries
