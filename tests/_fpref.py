"""numpy restatement of the 128-bit buffer digest `pg_fingerprint` computes on the device (definition: the header comment of
pigeon_amd/csrc/fingerprint.hip).  uint64 arithmetic wraps modulo 2^64, which is what numpy's unsigned arrays do.

    mix(z):   z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
    chunk i of ceil(bytes / 16) (little-endian words lo_i, hi_i; the last chunk zero padded):
        k_i = mix(seed + i + 1);   A += mix(lo_i ^ k_i);   B += mix(hi_i ^ rotl(k_i, 32))
    t = mix(seed ^ 0x9E3779B97F4A7C15);   out = (mix(A + t + bytes), mix(B + rotl(t, 32) + bytes))
"""
import numpy as np

_U = np.uint64
_M1, _M2, _G = _U(0xBF58476D1CE4E5B9), _U(0x94D049BB133111EB), _U(0x9E3779B97F4A7C15)


def _mix(z):
    z = np.asarray(z, dtype=_U).copy()
    z ^= z >> _U(30)
    z *= _M1
    z ^= z >> _U(27)
    z *= _M2
    z ^= z >> _U(31)
    return z


def _rotl32(z):
    z = np.asarray(z, dtype=_U)
    return (z << _U(32)) | (z >> _U(32))


def fingerprint(data, seed: int = 0):
    """data: bytes / bytearray / a numpy array (its bytes in memory order) -> (out0, out1) as Python ints."""
    raw = np.frombuffer(bytes(data) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).tobytes(), dtype=np.uint8)
    nbytes = int(raw.size)
    n = (nbytes + 15) // 16
    seed = _U(int(seed) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        A = B = _U(0)
        if n:
            pad = np.zeros(n * 16, dtype=np.uint8)
            pad[:nbytes] = raw
            w = pad.view("<u8").reshape(n, 2)
            k = _mix(seed + np.arange(1, n + 1, dtype=_U))
            A = _mix(w[:, 0] ^ k).sum(dtype=_U)
            B = _mix(w[:, 1] ^ _rotl32(k)).sum(dtype=_U)
        t = _mix(seed ^ _G)
        o0 = _mix(A + t + _U(nbytes))
        o1 = _mix(B + _rotl32(t) + _U(nbytes))
    return int(o0), int(o1)


def fingerprint_slow(data: bytes, seed: int = 0):
    """The same definition in plain Python integers, chunk by chunk (checks the vectorised form above on small inputs)."""
    M = (1 << 64) - 1

    def mix(z):
        z &= M
        z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & M
        z ^= z >> 27; z = (z * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    def rotl32(z):
        return ((z << 32) | (z >> 32)) & M

    data = bytes(data)
    A = B = 0
    for i in range((len(data) + 15) // 16):
        c = data[16 * i:16 * i + 16].ljust(16, b"\0")
        k = mix(seed + i + 1)
        A = (A + mix(int.from_bytes(c[:8], "little") ^ k)) & M
        B = (B + mix(int.from_bytes(c[8:], "little") ^ rotl32(k))) & M
    t = mix((seed & M) ^ 0x9E3779B97F4A7C15)
    return mix(A + t + len(data)), mix(B + rotl32(t) + len(data))
