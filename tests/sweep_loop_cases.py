"""Inputs that steer la_bdsqr3 (csrc/rtg_math.cuh), the 3x3 SBDSQR of the Kabsch fits, down each of its paths.

The 3-point fit with Z = (e_x, e_y, e_z) has A = M^T Z = M^T.  An upper-bidiagonal A (zero subdiagonal, zero A(0,2))
passes SGEBD2 with every tau = 0 (each SLARFG sees a zero tail), so (d1, d2, d3; e1, e2) reach SBDSQR exactly as set:
M = [[d1, 0, 0], [e1, d2, 0], [0, e2, d3]].  Thresholds are restated here in float32, operation for operation, so that
a case can sit on a threshold and on its float neighbours.

"Chase order" is the order the sweep works in: (D1, D2, D3; E1, E2) = (d1, d2, d3; e1, e2) for a top-to-bottom chase
(|d1| >= |d3|) and (d3, d2, d1; e2, e1) for a bottom-to-top one.  Either way |D1| >= |D3|.
"""
import numpy as np

F = np.float32
EPS = F(5.96046448e-08)
TOL = F(10.0) * EPS
UNFL = F(1.17549435e-38)
SQRT3 = F(1.73205078)


# Chase-order bidiagonals by the number of sweeps SBDSQR needs on them, the same number in either chase direction
# (found by a search with a counting build of the oracle; profiles/r16/path_coverage.txt has the counts).
SWEEPS_NEEDED = {
    1: [(1.92579293, -1.26127958, -0.773801208, 0.064267002, 0.0132922456),
        (1.97487605, -1.35162306, 0.483462512, 0.0103177652, -0.315214425),
        (1.31761873, -1.02787781, -0.605360448, -0.278337806, -0.00219461811),
        (-1.69548976, 1.63899815, -1.09253097, 0.0371988751, -0.0341791883),
        (1.8989979, 1.02174747, 0.542809308, -0.110401206, 0.0453956611),
        (-1.28366673, 0.556586742, 0.36378926, -0.0021947613, 0.0283191111),
        (0.603763044, 0.32810387, 0.0971409082, 0.0545575246, -0.0245577227),
        (1.49757004, 1.14108777, 0.265292346, 0.0131459506, 0.197601765)],
    2: [(0.88995111, -0.728755116, 0.233443961, -0.385189384, 0.544177175),
        (1.4064666, -0.410350561, 0.352250487, -0.0239338782, 0.140031263),
        (0.82007575, -0.592090666, 0.368996918, 0.495729268, -0.753330052),
        (-1.55035937, 0.800245941, -0.320518732, 0.450491756, -0.642550647),
        (-1.61376882, 1.47327542, -1.36425328, 6.03222084, -8.65073013),
        (1.89408183, -0.804749846, -0.0629037172, 3.23227739, 2.34036922),
        (1.6150527, 1.54106283, -1.34995353, -0.126429319, 0.0673320889),
        (-0.947482169, 0.442561567, 0.433786273, 0.0115187783, -0.162089512)],
    3: [(-0.769227326, -0.400360167, 0.204765648, 1.06275952, 0.0798235834),
        (-1.02767193, -0.671266437, -0.481010705, 2.35544872, 1.42030716),
        (1.90426981, -1.08454418, 0.809149921, -2.10049987, -0.231605858),
        (1.29663241, 1.06826258, -0.8373487, -0.682597041, -0.619024158),
        (1.36213613, 1.29091513, 0.588781655, -4.60223293, -1.74959099),
        (1.80234373, -1.42062604, -1.38914847, -1.00235069, 0.602350354),
        (-1.7260927, 1.70392573, -1.12111497, -6.57893372, 2.81547785),
        (1.66864741, 1.13766515, -0.414031953, 10.4986277, 2.03200102)],
    4: [(-1.51004195, -0.981785655, -0.751495481, -7.79438829, 1.23340607),
        (-1.82338297, 1.82074142, 1.78697848, -0.147300497, -0.0284614619),
        (1.07843637, -0.341065347, -0.13728492, 1.40198815, -0.429842353),
        (-1.67390871, -0.566923976, -0.269154996, 4.27863741, 0.725149691),
        (1.82354474, -0.71392858, 0.206829786, 2.23684835, 0.92655772),
        (-1.66418684, -1.64584053, -1.53287029, -1.21540153, -0.140649468),
        (-1.32585549, 1.3142494, -1.28190696, 0.637988567, -0.318244219),
        (1.24820352, -0.80541712, -0.689208925, -8.33201027, -0.895784974)],
    5: [(-1.51384866, -1.50901544, -1.50583112, -0.276089847, 0.0110622467),
        (-1.765275, 0.973683238, -0.328956753, 4.62186289, -0.713560939)],
}


def nb(x, k):
    """The float32 k steps above (k > 0) or below (k < 0) x."""
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def thresh(d1, d2, d3, e1, e2):
    """SBDSQR's THRESH = max(tol sminoa / sqrt(3), 18 unfl) for the bidiagonal in index order."""
    d1, d2, d3, e1, e2 = (F(v) for v in (d1, d2, d3, e1, e2))
    s = abs(d1)
    if s != 0:
        mu = abs(d2) * (s / (s + abs(e1)))
        s = min(s, mu)
        if s != 0:
            mu = abs(d3) * (mu / (mu + abs(e2)))
            s = min(s, mu)
    s = s / SQRT3
    return max(TOL * s, F(6.0) * (F(3.0) * (F(3.0) * UNFL)))


def place(c, mir):
    """Chase-order (D1, D2, D3, E1, E2) -> index order (d1, d2, d3, e1, e2) for the given direction."""
    D1, D2, D3, E1, E2 = c
    return (D3, D2, D1, E2, E1) if mir else (D1, D2, D3, E1, E2)


def _at_thresh(d, other_e, which):
    """e_which on THRESH (a fixed point: THRESH depends on e itself) for d = (d1, d2, d3) and the other e given."""
    e = F(1e-8)
    for _ in range(6):
        t = (d[0], d[1], d[2], other_e, e) if which == 2 else (d[0], d[1], d[2], e, other_e)
        e = thresh(*t)
    return e


def chase_cases():
    """[(label, (D1, D2, D3, E1, E2))] with |D1| > |D3|: every case is valid for both chase directions."""
    out = []
    bases = [(1.0, 0.7, 0.4, 0.3), (-1.25, 0.6, -0.35, -0.2), (3.0, -1.5, 0.9, 0.8)]
    for b, (D1, D2, D3, E1) in enumerate(bases):
        # convergence test 1, |E2| <= tol |D3|: just true (k <= 0: E2 zeroed, no sweep this pass) and just false
        t = TOL * abs(F(D3))
        for k in (-2, -1, 0, 1, 2):
            for sg in (1, -1):
                out.append((f"conv1 base{b} k={k}", (D1, D2, D3, E1, sg * nb(t, k))))
        # convergence test 2, |E1| <= tol |D1| (test 1 false: E2 is ordinary): E1 zeroed / not
        t = TOL * abs(F(D1))
        for k in (-2, -1, 0, 1, 2):
            for sg in (1, -1):
                out.append((f"conv2 base{b} k={k}", (D1, D2, D3, sg * nb(t, k), 0.25)))
        # convergence test 3, |E2| <= tol mu2 with mu2 = |D2| (|D1| / (|D1| + |E1|)); test 1 stays false because
        # |D3| is far below mu2
        d3 = F(D3) * F(0.01)
        mu = abs(F(D1))
        mu = abs(F(D2)) * (mu / (mu + abs(F(E1))))
        t = TOL * mu
        for k in (-2, -1, 0, 1, 2):
            for sg in (1, -1):
                out.append((f"conv3 base{b} k={k}", (D1, D2, d3, E1, sg * nb(t, k))))
    # the zero-shift sweep: a zero in d makes smin = 0 (D3 = 0, D2 = 0) -- the first pass sweeps without a shift
    for D in ((1.0, 0.7, 0.0), (1.0, 0.0, 0.4), (1.0, 0.0, 0.0), (-2.0, 0.5, -0.0)):
        for E in ((0.3, 0.2), (-0.4, 0.1), (1e-3, 0.9)):
            out.append(("zero in d: zero-shift sweep", D + E))
    # well-separated values, ordinary e: smin / smax is far above eps / (3 tol), so the sweep is shifted
    for D in ((3.0, 1.0, 0.2), (8.0, -2.0, 0.5), (1.0, 0.5, 0.25)):
        for E in ((0.5, 0.4), (-0.1, 0.3), (0.9, -0.05)):
            out.append(("well separated: shifted sweep", D + E))
    # the shift dropped because q q < eps, q = shift / |D1|: no 3x3 reaches it.  The test is only made when
    # smin / smax > eps / (3 tol) = 1 / 30; smin <= |D2|, |D3|, and the 2x2's smallest singular value is
    # shift = |D2 D3| / sigma_max >= |D2 D3| / (sqrt(3) smax) > smax / 1559, so q >= shift / smax > 6.4e-4 and
    # q q > 4e-7 > eps.  These sit as near that corner as the bounds allow (both come out as ordinary sweeps)
    for s in (2.0e-4, 2.4e-4, 2.5e-4, 1e-3):
        out.append(("q q < eps candidates", (1.0, 1.0, s, 1e-6, 1e-6)))
        out.append(("q q < eps candidates", (1.0, s, s * 0.5, 0.5, s)))
    # lanes needing different numbers of sweeps: the smaller e is, the sooner a convergence test fires
    rng = np.random.default_rng(1616)
    for i in range(192):
        d = np.sort(rng.uniform(0.05, 2.0, 3))[::-1] * rng.choice([-1.0, 1.0], 3)
        e = rng.normal(size=2) * 2.0 ** -rng.integers(0, 24)
        out.append((f"sweep count e~2^-{i % 24}", (d[0], d[1], d[2], e[0], e[1])))
    for k, cs in SWEEPS_NEEDED.items():
        for c in cs:
            out.append((f"{k} sweeps", c))
    return [(lab, tuple(F(v) for v in c)) for lab, c in out]


def index_cases():
    """[(label, (d1, d2, d3, e1, e2))] in index order: chase direction ties, deflation, split, SGESDD's rescaling."""
    out = []
    # equal magnitudes: |d1| >= |d3| holds, so top to bottom; one step either side flips it
    for d1, d3 in ((0.7, 0.7), (0.7, -0.7), (-0.7, 0.7), (-0.7, -0.7)):
        for k in (-1, 0, 1):
            out.append((f"|d1| = |d3| k={k}", (d1, 0.5, np.copysign(nb(abs(d3), k), d3), 0.3, 0.2)))
    for d in ((1.0, 0.7, 0.4), (0.4, 0.7, 1.0), (0.7, -0.5, 0.7), (-1.5, 2.0, 3.0)):
        # e2 at and about THRESH (k <= 0: deflation, block (1, 2); above: the full block), e2 zero and tiny
        t = _at_thresh(d, 0.3, 2)
        for e2 in [nb(t, k) for k in (-2, -1, 0, 1, 2)] + [F(0.0), F(-0.0), F(1e-30), F(-1e-41)]:
            for sg in (1, -1):
                out.append(("e2 about thresh: deflation to block (1, 2)", d + (0.3, sg * e2)))
        # both e at or below THRESH: deflation, then |e1| <= thresh ends it with no block
        t1 = _at_thresh(d, 0.0, 1)
        for e1 in [nb(t1, k) for k in (-2, -1, 0, 1, 2)] + [F(0.0), F(-1e-35)]:
            for e2 in (F(0.0), F(1e-33), nb(_at_thresh(d, e1, 2), -1)):
                out.append(("both e about thresh: no block / block (1, 2)", d + (e1, e2)))
        # e1 at and about THRESH with an ordinary e2: the split at E(1), block (2, 3)
        t = _at_thresh(d, 0.3, 1)
        for e1 in [nb(t, k) for k in (-2, -1, 0, 1, 2)] + [F(0.0), F(-0.0), F(1e-30)]:
            for sg in (1, -1):
                out.append(("e1 about thresh: split to block (2, 3)", d + (sg * e1, 0.3)))
    # a zero d1 (thresh = 18 unfl, bottom to top), alone and with other zeros
    for d in ((0.0, 0.7, 0.4), (0.0, 0.0, 0.4), (0.0, 0.7, 0.0), (-0.0, 0.0, 0.0)):
        out.append(("d1 = 0", d + (0.3, 0.2)))
    # anrm = max |A| on both sides of 2^+-40 (SGESDD rescales beyond, strictly): whole binades and float neighbours
    for base in ((1.0, 0.7, 0.4, 0.3, 0.2), (0.4, -0.7, 1.0, 0.3, -0.2)):
        for k in list(range(-44, -36)) + list(range(37, 45)):
            out.append((f"anrm = 2^{k}", tuple(np.ldexp(F(v), k) for v in base)))
        for k in (-40, 40):
            for j in (-1, 1):
                sc = tuple(np.ldexp(F(v), k) for v in base)
                out.append((f"anrm next to 2^{k}", tuple(nb(v, j) if abs(v) == np.ldexp(F(1.0), k) else v for v in sc)))
    return [(lab, tuple(F(v) for v in c)) for lab, c in out]


def hostile_cases():
    """NaN and +-inf in each of the five entries (the fit's einsum turns an inf into NaNs elsewhere in A: inf * 0):
    the sweep loop runs such a lane to its iteration cap."""
    out = []
    for pos in range(5):
        for v in (np.nan, np.inf, -np.inf):
            c = [1.0, 0.7, 0.4, 0.3, 0.2]
            c[pos] = v
            out.append((f"{v} at entry {pos}", tuple(F(x) for x in c)))
    return out


def bidiag_points(de):
    """(n, 5) index-order (d1, d2, d3, e1, e2) -> (Z, M), each (n, 3, 3): the 3-point fit whose A is that bidiagonal."""
    de = np.asarray(de, np.float32).reshape(-1, 5)
    n = len(de)
    M = np.zeros((n, 3, 3), np.float32)
    M[:, 0, 0], M[:, 1, 1], M[:, 2, 2] = de[:, 0], de[:, 1], de[:, 2]
    M[:, 1, 0], M[:, 2, 1] = de[:, 3], de[:, 4]
    Z = np.broadcast_to(np.eye(3, dtype=np.float32), (n, 3, 3)).copy()
    return Z, M


def bidiag_frames():
    """All cases as one batch of index-order rows with a label each: the chase cases top to bottom in whole waves,
    bottom to top in whole waves, the two alternating lane by lane, the index-order cases, one wave whose lanes need
    1, 2, 3 and 4 sweeps, and ordinary lanes with NaN / inf lanes at positions 0 and 63 of each 64."""
    ch = chase_cases()
    rows, labels = [], []

    def add(lab, c):
        rows.append(c)
        labels.append(lab)

    def pad():   # to a whole wave, with ordinary lanes
        while len(rows) % 64:
            add("pad", (F(1.0), F(0.7), F(0.4), F(0.3), F(0.2)))

    for mir in (False, True):
        for lab, c in ch:
            add(f"{'bottom-up' if mir else 'top-down'} wave: {lab}", place(c, mir))
        pad()
    for i, (lab, c) in enumerate(ch):                     # lane 2i top-down, lane 2i + 1 bottom-up
        add(f"alternating, top-down: {lab}", place(c, False))
        add(f"alternating, bottom-up: {lab}", place(ch[(i + 7) % len(ch)][1], True))
    pad()
    for lab, c in index_cases():
        add(lab, c)
    pad()
    for i in range(64):                                   # one wave whose lanes need 1, 2, 3, 4 sweeps, lane by lane
        k = 1 + i % 4
        add(f"mixed wave: {k} sweeps", place(tuple(F(v) for v in SWEEPS_NEEDED[k][(i // 4) % 8]), bool((i // 4) & 1)))
    ho = hostile_cases()
    for i in range(64 * ((len(ho) + 1) // 2)):
        if i % 64 in (0, 63):
            lab, c = ho[(i // 64) * 2 + (i % 64 == 63)] if (i // 64) * 2 + (i % 64 == 63) < len(ho) else ho[0]
            add(f"hostile lane {i % 64}: {lab}", c)
        else:
            lab, c = ch[(5 * i) % len(ch)]
            add(f"beside a hostile lane: {lab}", place(c, bool(i & 1)))
    return np.array(rows, np.float32), labels
