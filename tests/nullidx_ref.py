"""CPU restatement of the genome window index, written for the tests from the definition:

  per byte   na = byte in nN, cg = byte in cgCG, rp = byte in acgt; any other byte sets no flag
  windows    the starts i in [0, T - t); NA_i, CG_i, RP_i = the flags summed over [i, i + t)
  indexed    iff NA_i == 0, under the key CG_i (t + 1) + RP_i
  pos        the indexed starts by key, ascending inside a key
  ptr[c][r]  the number of indexed windows with a smaller key
  planes     numpy.packbits of each flag

`index_direct` recounts every window (small T); `index_vectorised` uses cumulative sums, a stable argsort and bincount.
`write_index` lays the files out as gkmqc_amd.nullseq.build_index does, so that the host tests need no device."""
import os

import numpy as np

NOKEY = 0xFFFFFFFF


def as_bytes(seq):
    if isinstance(seq, str):
        seq = seq.encode()
    if isinstance(seq, (bytes, bytearray)):
        return np.frombuffer(bytes(seq), dtype=np.uint8)
    return np.ascontiguousarray(seq, dtype=np.uint8)


def flags(raw):
    raw = as_bytes(raw)
    return (np.isin(raw, np.frombuffer(b"nN", np.uint8)), np.isin(raw, np.frombuffer(b"cgCG", np.uint8)),
            np.isin(raw, np.frombuffer(b"acgt", np.uint8)))


def _finish(raw, t, key):
    na, cg, rp = flags(raw)
    cells = (t + 1) ** 2
    ok = key != NOKEY
    starts = np.nonzero(ok)[0]
    order = np.argsort(key[ok], kind="stable")
    counts = np.bincount(key[ok].astype(np.int64), minlength=cells)
    ptr = np.zeros(cells, np.int64)
    np.cumsum(counts[:-1], out=ptr[1:])
    return dict(key=key, pos=starts[order].astype(np.int32), ptr=ptr.astype(np.int32).reshape(t + 1, t + 1),
                len=int(ok.sum()), na=np.packbits(na), cg=np.packbits(cg), rp=np.packbits(rp))


def index_direct(raw, t):
    """Every window recounted from its own bytes."""
    raw = as_bytes(raw)
    T = len(raw)
    key = np.zeros(max(0, T - t), np.uint32)
    for i in range(max(0, T - t)):
        w = raw[i:i + t].tobytes()
        n = sum(w.count(c) for c in b"nN")
        c = sum(w.count(c) for c in b"cgCG")
        r = sum(w.count(c) for c in b"acgt")
        key[i] = NOKEY if n else c * (t + 1) + r
    return _finish(raw, t, key)


def index_vectorised(raw, t):
    raw = as_bytes(raw)
    T = len(raw)
    nwin = max(0, T - t)
    sums = []
    for f in flags(raw):
        s = np.zeros(T + 1, np.int64)
        np.cumsum(f, out=s[1:])
        sums.append(s[t:t + nwin] - s[:nwin])
    key = (sums[1] * (t + 1) + sums[2]).astype(np.uint32)
    key[sums[0] > 0] = NOKEY
    return _finish(raw, t, key)


def write_index(out_dir, width, records, index=index_vectorised):
    """records: [(name, raw letters)] -> the files of an index directory."""
    for sub in ("fa", "bit", "nidx_t%d" % width):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    for name, raw in records:
        raw = as_bytes(raw)
        ix = index(raw, width)
        with open(os.path.join(out_dir, "fa", name + ".fa"), "wb") as f:
            f.write(b">" + name.encode() + b"\n")
            for a in range(0, len(raw), 50):
                f.write(raw[a:a + 50].tobytes() + b"\n")
        for pl in ("na", "cg", "rp"):
            ix[pl].tofile(os.path.join(out_dir, "bit", "%s.%s.bit" % (name, pl)))
        np.save(os.path.join(out_dir, "nidx_t%d" % width, name + "_pos.npy"), ix["pos"])
        np.savez_compressed(os.path.join(out_dir, "nidx_t%d" % width, name + "_ptr.npz"), ptr=ix["ptr"], len=ix["len"])


def soft_masked(T, seed, n_gaps=3, gap=700, gc=0.42):
    """A seeded chromosome-like byte string: ACGT with repeat runs in lower case and a few runs of N."""
    rng = np.random.default_rng(seed)
    p = np.array([(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2])
    raw = np.frombuffer(b"ACGT", np.uint8)[rng.choice(4, size=T, p=p)].copy()
    a = 0
    while a < T:                      # alternate unique stretches and repeat runs
        a += int(rng.integers(50, 3000))
        b = min(T, a + int(rng.integers(20, 1500)))
        raw[a:b] |= 0x20
        a = b
    for _ in range(n_gaps):
        a = int(rng.integers(0, max(1, T - gap)))
        raw[a:a + int(rng.integers(1, gap + 1))] = ord("N")
    return raw
