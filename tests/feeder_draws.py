"""numpy restatement of the device feeder's draw stream (include/tamgcn.h, tamgcn_feeder_draw; INTEGRATION.md
"Training loop"), vectorised over the batch slots.  Test infrastructure: tests/test_feeder_draw_cpu.py holds it to
Philox known answers and to the distributions of the reference's recipe, tests/test_gpu_feeder_draw.py holds the kernel
to it bit for bit."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints -> four uint64 arrays holding 32-bit words."""
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                  # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def _blocks(seed, call, B, j):
    slot, zero = np.arange(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)
    counter = (zero + np.uint64(call & 0xFFFFFFFF), zero + np.uint64((call >> 32) & 0xFFFFFFFF), slot, zero + np.uint64(j))
    return philox4x32_10(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def draws(seed, call, lengths, time_steps=52):
    """Slot b of call `call` under `seed`, for a clip of lengths[b] frames.  Returns agx, agy (int64 [B]), s (float64 [B]),
    idx (int32 [B, time_steps], sorted) and the positions Floyd's algorithm took (int64 [B, time_steps])."""
    L = np.asarray(lengths, dtype=np.int64).reshape(-1)
    B = L.size
    w = _blocks(seed, call, B, 0)
    agx = -60 + ((w[0] * np.uint64(121)) >> _S32).astype(np.int64)
    agy = -60 + ((w[1] * np.uint64(121)) >> _S32).astype(np.int64)
    s = 0.5 + ((w[2] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w[3] >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    u = np.concatenate([np.stack(_blocks(seed, call, B, j), axis=1) for j in range(1, (time_steps + 3) // 4 + 1)], axis=1)
    n = 100 * L
    pos = np.zeros((B, time_steps), dtype=np.int64)
    for i in range(time_steps):                          # Floyd: a uniform time_steps-subset of range(n)
        J = n - time_steps + i
        t = ((u[:, i] * (J + 1).astype(np.uint64)) >> _S32).astype(np.int64)
        taken = (pos[:, :i] == t[:, None]).any(axis=1)
        pos[:, i] = np.where(taken, J, t)
    idx = np.sort(pos % L[:, None], axis=1).astype(np.int32)
    return agx, agy, s, idx, pos


def val_indices(length, time_steps=52):
    """np.linspace(0, length - 1, time_steps).astype(int) spelled out the way the kernel computes it."""
    if time_steps == 1:
        return np.zeros(1, dtype=np.int64)
    step = np.float64(length - 1) / np.float64(time_steps - 1)
    out = (np.arange(time_steps, dtype=np.float64) * step).astype(np.int64)
    out[-1] = length - 1
    return out
