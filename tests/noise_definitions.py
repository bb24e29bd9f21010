"""Float64 definition of the noise estimate, from the textbook formulas, and the bound on what binary32 evaluation may differ from it.

Definition (inputs: the binary32 bucket words, the binary32 scale, floor and luma weights, all taken as exact reals):
    Y_j = scale (0.2126f r_j + 0.7152f g_j + 0.0722f b_j)          M = (1/k) sum Y_j          D_j = Y_j - M
    VAR = sum D_j^2 / (k - 1)          SE = sqrt(VAR / k)          E = SE / (M + floor)   (0 where M + floor = 0)

Bound, for non-negative words without overflow or underflow, u = 2^-24, first order in u (hats = the binary32 values of noise_twin):
  y    three products and two sums of non-negative terms, then the scale: 4 roundings, |y^_j - Y_j| <= 4u Y_j.
  mean k - 1 sequential additions of non-negative terms and one division: m^ = mean(y^)(1 + t), |t| <= k u; mean(y^) inherits 4u:
       |m^ - M| <= (k + 4) u M.
  d    one subtraction: |d^_j - D_j| <= 4u Y_j + (k + 4) u M + u |D_j| <= (k + 9) u Ymax, with Ymax = max_j Y_j >= M and |D_j| <= Ymax.
  se   as a function of the vector d it is |d|_2 / sqrt(k (k - 1)), Lipschitz: |se(d^) - se(D)| <= sqrt(k) max_j|d^_j - D_j| / sqrt(k (k - 1))
       <= (k + 9) u Ymax.  Its own arithmetic: k squares (u each), k - 1 additions of non-negative terms, two divisions — (k + 2) u
       relative on var / k, half of that after the root — and the root's u: (k/2 + 2) u SE.
  e    denominator m^ + floor: |.| <= (k + 4) u M + u (M + floor) <= (k + 5) u (M + floor); the division: u.  Together (k + 6) u E,
       and E = SE / (M + floor).
  sum  |e^ - E| <= ((k + 9) u Ymax + (1.5 k + 8) u SE) / (M + floor).
The terms of second order are below (2k + 20)^2 u^2 (Ymax + SE) / (M + floor) < 2e-4 u (Ymax + SE) / (M + floor) for k <= 16; both
constants are raised by one to cover them (and float64's own rounding, 2^-29 u):

    |e^ - E| <= ((k + 10) u Ymax + (1.5 k + 9) u SE) / (M + floor)

The first term dominates where the buckets agree (SE << Ymax): there E itself is small and what is bounded is an absolute error of a few
u Ymax / (M + floor) — the cancellation in y_j - mean."""
import numpy as np

f64 = np.float64
u = 2.0 ** -24
LUMA64 = tuple(f64(np.float32(c)) for c in (0.2126, 0.7152, 0.0722))


def noise_e64(slab, scale, floor):
    """slab [tiles][k][3][256] -> dict of float64 arrays [tiles][256]: e, se, mean, ymax."""
    s = np.asarray(slab, dtype=np.float32).astype(f64)
    k = s.shape[1]
    y = f64(np.float32(scale)) * (LUMA64[0] * s[:, :, 0] + LUMA64[1] * s[:, :, 1] + LUMA64[2] * s[:, :, 2])      # [tiles][k][256]
    mean = y.mean(axis=1)
    var = ((y - mean[:, None, :]) ** 2).sum(axis=1) / (k - 1)
    se = np.sqrt(var / k)
    denom = mean + f64(np.float32(floor))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(denom == 0.0, 0.0, se / denom)
    return {"e": e, "se": se, "mean": mean, "ymax": y.max(axis=1), "denom": denom}


def bound(d, k):
    """The bound of the module docstring on |binary32 e - float64 e|, per pixel."""
    return ((k + 10) * u * d["ymax"] + (1.5 * k + 9) * u * d["se"]) / d["denom"]
