"""numpy restatement of include/sship.h "Image pyramid": integers only.  `down` is the separable form (a horizontal pass, then a vertical
one); `down_direct` evaluates the 25 taps of the text one by one.  tests/test_pyr_cpu.py holds the two equal."""
from __future__ import annotations

import numpy as np

K5 = (1, 4, 6, 4, 1)


def reflect101(i: int, n: int) -> int:
    """r(i, n) of the rule: r(i, 1) = 0; otherwise i < 0 -> -i and i >= n -> 2 (n - 1) - i, repeated until the index is inside"""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def level_shapes(h: int, w: int, levels: int):
    out = [(h, w)]
    for _ in range(1, levels):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def _taps(n: int):
    """index array [(n + 1) // 2, 5]: the source index of tap j = -2 .. 2 of output y"""
    return np.array([[reflect101(2 * y + j, n) for j in range(-2, 3)] for y in range((n + 1) // 2)], np.int64)


def down(img: np.ndarray) -> np.ndarray:
    """u8 [h, w] -> u8 [(h + 1) // 2, (w + 1) // 2]"""
    s = np.asarray(img).astype(np.int64)
    h, w = s.shape
    k = np.array(K5, np.int64)
    hor = (s[:, _taps(w)] * k).sum(axis=2)                                        # [h, w']  <= 16 * 255
    acc = (hor[_taps(h), :] * k[None, :, None]).sum(axis=1)                       # [h', w'] <= 65 280
    assert acc.max(initial=0) <= 65280
    return ((acc + 128) >> 8).astype(np.uint8)


def down_direct(img: np.ndarray) -> np.ndarray:
    """the text's double sum, tap by tap"""
    s = np.asarray(img)
    h, w = s.shape
    out = np.empty(((h + 1) // 2, (w + 1) // 2), np.uint8)
    for y in range(out.shape[0]):
        for x in range(out.shape[1]):
            acc = 0
            for j in range(-2, 3):
                for i in range(-2, 3):
                    acc += K5[j + 2] * K5[i + 2] * int(s[reflect101(2 * y + j, h), reflect101(2 * x + i, w)])
            out[y, x] = (acc + 128) >> 8
    return out


def build(imgs: np.ndarray, levels: int):
    """u8 [n, h, w] -> [level 0 (the input), level 1, ...], each u8 [n, h_l, w_l]"""
    out = [np.asarray(imgs)]
    for _ in range(1, levels):
        out.append(np.stack([down(im) for im in out[-1]]))
    return out
