"""Python twin of gpsh::RandomSelector (host/random_selector.hpp): the uniform branch of the reference's RandomSelector
(include/dataset_reader.h:26-100) -- draw an index into the remaining list, take the element, swap with the back and pop, refill
when empty -- with the generator and the draw written out so that both hosts give the same order:
  * MT19937 (std::mt19937) seeded with the low 32 bits of `seed`;
  * one 32-bit output r at a time, rejected while r >= 2^32 - 2^32 mod n, then r mod n.
"""


class MT19937:
    """std::mt19937: 32-bit Mersenne Twister, seeded by the linear recurrence of its constructor (init_genrand)"""

    def __init__(self, seed=5489):
        mt = [0] * 624
        mt[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            mt[i] = (1812433253 * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.mt, self.index = mt, 624

    def _twist(self):
        mt = self.mt
        for i in range(624):
            y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
            mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
        self.index = 0

    def __call__(self):
        if self.index >= 624:
            self._twist()
        y = self.mt[self.index]
        self.index += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


def draw_below(gen, n):
    """unbiased draw on [0, n), n in [1, 2^32], from 32-bit outputs of `gen`"""
    zone = (1 << 32) - (1 << 32) % n
    while True:
        r = gen()
        if r < zone:
            return r % n


class RandomSelector:
    def __init__(self, items, seed):
        if len(items) == 0:
            raise ValueError("RandomSelector: no items")
        self.original = [(v, i) for i, v in enumerate(items)]
        self.current = list(self.original)
        self.gen = MT19937(seed & 0xFFFFFFFF)

    def getNext(self):
        """-> (value, originalIndex)"""
        if not self.current:
            self.current = list(self.original)
        i = draw_below(self.gen, len(self.current))
        v = self.current[i]
        self.current[i] = self.current[-1]
        self.current.pop()
        return v
