"""NumPy restatement of the vocabulary trainer's fixed arithmetic (include/sfmloc.h, sfmloc_bowtrain_*): cv::RNG, the
getRandomTrainFeatures draws, the PCA moments, and cv::kmeans (k-means++ seeding, Lloyd, the empty-cluster rule, best of
the attempts) with the chunked f64 sums the device uses.  Slow (Python loops over the seeding): small samples only."""
import numpy as np

CHUNK = 1024
U32 = 0xFFFFFFFF


class CvRng:
    """cv::RNG: multiply-with-carry, state 0 means 0xffffffff"""

    def __init__(self, state=0xFFFFFFFF):
        self.state = int(state) or 0xFFFFFFFF

    def next(self):
        self.state = ((self.state & U32) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & U32

    def uniform01(self):  # uniform(0.f, 1.f)
        return np.float32(np.float32(self.next()) * np.float32(2.3283064365386962890625e-10))

    def double(self):  # (double)rng
        t = self.next()
        lo = self.next()
        return float(((t << 32) | lo)) * 5.4210108624275221700372640043497e-20


def draw_index(n, r):
    """(int)(n * r) in float32, clamped below n"""
    k = int(np.float32(np.float32(n) * np.float32(r)))
    return min(k, n - 1)


def pca_moments(x):
    """integer-exact moments -> (mean, cov) by the stated f64 formula"""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    sx = x.sum(0)
    sxx = x.T @ x
    mean = sx / n
    cov = (sxx - n * np.outer(mean, mean)) / n
    return mean, cov


def sign_rule(vecs_rows):
    v = np.array(vecs_rows, np.float64)
    for r in range(v.shape[0]):
        big = int(np.argmax(np.abs(v[r])))
        if v[r, big] < 0:
            v[r] = -v[r]
    return v


def dist_f32(x, c):
    """[n, d] x [k, d] -> [n, k]: sum_d (x_d - c_d)^2 in f32, dimension order, unfused"""
    x = np.asarray(x, np.float32)
    c = np.asarray(c, np.float32)
    s = np.zeros((x.shape[0], c.shape[0]), np.float32)
    for d in range(x.shape[1]):
        t = x[:, d, None] - c[None, :, d]
        s = s + t * t
    return s


def chunk_partials(v):
    v = np.asarray(v, np.float64)
    return np.array([np.cumsum(v[i:i + CHUNK])[-1] for i in range(0, v.shape[0], CHUNK)], np.float64)


def seq_sum(p):
    return float(np.cumsum(np.asarray(p, np.float64))[-1]) if len(p) else 0.0


def pp_draw(dist, u):
    part = chunk_partials(dist)
    total = seq_sum(part)
    target = u * total
    before = 0.0
    for c, pc in enumerate(part):
        end = before + pc
        if end >= target:
            q = np.cumsum(np.asarray(dist[c * CHUNK:(c + 1) * CHUNK], np.float64))
            hit = np.nonzero(before + q >= target)[0]
            if hit.size:
                return c * CHUNK + int(hit[0])
            break
        before = end
    return dist.shape[0] - 1


def centers_pp(x, K, rng):
    n = x.shape[0]
    ids = [rng.next() % n]
    dist = dist_f32(x, x[ids[0]][None])[:, 0]
    for _ in range(1, K):
        best_sum, best_c, best_d = np.inf, -1, None
        for _t in range(3):
            u = rng.double()
            ci = pp_draw(dist, u)
            d2 = np.minimum(dist_f32(x, x[ci][None])[:, 0], dist)
            s = seq_sum(chunk_partials(d2))
            if s < best_sum:
                best_sum, best_c, best_d = s, ci, d2
        ids.append(best_c)
        dist = best_d
    return x[np.array(ids)].copy()


def center_sums(x, labels, K):
    n, d = x.shape
    tot = np.zeros((K, d), np.float64)
    cnt = np.zeros(K, np.int64)
    for c0 in range(0, n, CHUNK):
        part = np.zeros((K, d), np.float64)
        np.add.at(part, labels[c0:c0 + CHUNK], np.asarray(x[c0:c0 + CHUNK], np.float64))
        tot = tot + part
        cnt += np.bincount(labels[c0:c0 + CHUNK], minlength=K)
    return tot, cnt


def kmeans(x, K, attempts=3, max_iter=100, eps=float(np.finfo(np.float32).eps), seed=0xFFFFFFFF, trace=None,
           want_min_dist=False):
    """-> (centers f32, labels i32, compactness[, min distances of the last assignment f32]); trace (a list) collects the
    clusters the empty rule refilled"""
    x = np.ascontiguousarray(x, np.float32)
    n = x.shape[0]
    K = min(K, n)
    rng = CvRng(seed)
    eps2 = max(eps, 0.0) ** 2
    best = (None, None, np.inf, None)
    for _a in range(attempts):
        it, max_shift = 0, np.inf
        cen = labels = mind = None
        while True:
            if it == 0:
                cen = centers_pp(x, K, rng)
            else:
                s, cnt = center_sums(x, labels, K)
                labels = labels.copy()
                for k in range(K):
                    if cnt[k] != 0:
                        continue
                    mk = int(np.argmax(cnt))  # first of the biggest
                    base = (s[mk] / cnt[mk]).astype(np.float32)
                    members = np.nonzero(labels == mk)[0]
                    dd = dist_f32(x[members], base[None])[:, 0]
                    far = int(members[np.nonzero(dd == dd.max())[0][-1]])
                    cnt[mk] -= 1
                    cnt[k] += 1
                    labels[far] = k
                    s[mk] = s[mk] - x[far].astype(np.float64)
                    s[k] = s[k] + x[far].astype(np.float64)
                    if trace is not None:
                        trace.append(k)
                new = (s / cnt[:, None].astype(np.float64)).astype(np.float32)
                t = new.astype(np.float64) - cen.astype(np.float64)
                sh = np.zeros(K)
                for d in range(x.shape[1]):
                    sh = sh + t[:, d] * t[:, d]
                max_shift = float(sh.max())
                cen = new
            it += 1
            if it == max(max_iter, 2) or max_shift <= eps2:
                break
            dm = dist_f32(x, cen)
            labels = np.argmin(dm, axis=1).astype(np.int32)
            mind = dm[np.arange(n), labels]
        comp = seq_sum(chunk_partials(mind))
        if comp < best[2]:
            best = (cen.copy(), labels.copy(), comp, mind.copy())
    return best if want_min_dist else best[:3]
