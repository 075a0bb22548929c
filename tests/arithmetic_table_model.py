"""A model of the DEVICE's division (csrc/arithmetic_table.hip, at_divide) on Python integers cut into 32-bit limbs, step for step
(TEST INFRASTRUCTURE ONLY): a numerator below 2^512 by a divisor in 1 .. 2^256 - 1. It exists to count the branches the kernel
takes, so that the instance list can be shown to take every one of them (tests/test_arithmetic_table_ref.py).

    1. the divisor is normalised to exactly eight limbs with the top bit set: conditional moves by 4, 2 and 1 limbs, then a bit
       shift by the leading zeros of limb 7; the numerator takes the same shift and grows to 24 limbs;
    2. sixteen quotient digits, most significant first. The window is nine limbs (the running remainder and the next numerator limb).
       The estimate is min((w8 2^32 + w7) / d7, 2^32 - 1); it is corrected at most twice by Knuth's test against d6
       (estimate * d6 > rhat 2^32 + w6, while rhat < 2^32); the eight-limb multiply-subtract follows, and an add-back where it
       borrowed;
    3. the remainder is shifted back.

Counters, per digit: the estimate was exact, one too large, two too large; and the add-backs."""

M32 = 0xFFFFFFFF


class Counters:
    def __init__(self):
        self.exact = self.one_too_large = self.two_too_large = self.add_back = 0
        self.limb_shift = [0] * 8  # by how many limbs the divisor was moved
        self.top_equal = 0         # w8 == d7: the estimate is cut to 2^32 - 1

    def as_dict(self):
        return dict(exact=self.exact, one_too_large=self.one_too_large, two_too_large=self.two_too_large, add_back=self.add_back)


def _limbs(x, n):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def _value(limbs):
    return sum(v << (32 * i) for i, v in enumerate(limbs))


def divide(numerator, divisor, counters=None):
    """(quotient, remainder) the way the kernel computes them"""
    c = counters if counters is not None else Counters()
    assert 0 <= numerator < 1 << 512 and 0 < divisor < 1 << 256
    d, n = _limbs(divisor, 8), _limbs(numerator, 16) + [0] * 8
    limb_shift = 0
    for k in (4, 2, 1):
        if not any(d[8 - k:]):
            d = [0] * k + d[: 8 - k]
            n = [0] * k + n[: 24 - k]
            limb_shift += k
    c.limb_shift[limb_shift] += 1
    bits = 32 - d[7].bit_length()
    if bits:
        d = [((d[i] << bits) | (d[i - 1] >> (32 - bits) if i else 0)) & M32 for i in range(8)]
        n = [((n[i] << bits) | (n[i - 1] >> (32 - bits) if i else 0)) & M32 for i in range(24)]
    r = n[16:]
    q = [0] * 16
    for j in range(15, -1, -1):
        w = [n[j]] + r  # nine limbs, below d 2^32
        num = (w[8] << 32) | w[7]
        if w[8] >= d[7]:
            c.top_equal += 1
            qhat = M32
        else:
            qhat = num // d[7]
        rhat = num - qhat * d[7]
        estimate = qhat
        for _ in range(2):
            if rhat <= M32 and qhat * d[6] > ((rhat << 32) | w[6]):
                qhat -= 1
                rhat += d[7]
        big = _value(w) - qhat * _value(d)  # the kernel's eight-limb multiply-subtract; a borrow out of limb 8 is big < 0
        if big < 0:
            c.add_back += 1
            qhat -= 1
            big += _value(d)
        assert 0 <= big < _value(d)
        w = _limbs(big, 9)
        q[j] = qhat
        over = estimate - qhat
        if over == 0:
            c.exact += 1
        elif over == 1:
            c.one_too_large += 1
        else:
            assert over == 2
            c.two_too_large += 1
        r = w[:8]
    rem = _value(r) >> bits
    assert rem >> (32 * limb_shift) << (32 * limb_shift) == rem
    return _value(q), rem >> (32 * limb_shift)
