"""Reference for the pooled egocentric observation (bcp_egocentric_costmaps_pooled): the maximum over every pool x pool
block of an image, edge blocks partial.  numpy only -- nothing from the product."""
import numpy as np


def block_max(img, pool):
    """img [..., H, W] uint8 -> [..., ceil(H / pool), ceil(W / pool)]: padded with zeros to a multiple of `pool` (a zero
    never wins a maximum of bytes, so padding stands for "nothing outside the image takes part"), reshaped, max."""
    img = np.asarray(img)
    h, w = img.shape[-2:]
    ph, pw = -(-h // pool), -(-w // pool)
    padded = np.zeros(img.shape[:-2] + (ph * pool, pw * pool), dtype=img.dtype)
    padded[..., :h, :w] = img
    return padded.reshape(img.shape[:-2] + (ph, pool, pw, pool)).max(axis=(-3, -1))
