"""mostLikeliBaseRead (src/assembler/correction.cpp:7-123) restated in np.longdouble, vectorised over pile-ups.

The tables come from tests/golden/functions/damage_dhigh.txt (the reference's own long double values).  The model is trusted only
through tests/test_correct_directed.py::test_model_reproduces_known_answers: it has to give the reference's answer on all 3000
recorded pile-ups of mostlikeli.tsv.gz.  It needs an x87 long double (x86-64): `usable()` says whether this machine has one.

A pile-up is {qBase, qIter, qLen, wasCorr, count[4][11], reverse[4][11]} (slot = target base * 11 + damage class).
"""
import gzip
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LD = np.longdouble
SMOOTH = 0.001


def usable():
    return np.finfo(LD).nmant == 63


def _ld(hexstr):
    """parse a C99 hex float literal exactly into a long double"""
    neg = hexstr.startswith("-")
    h = hexstr.lstrip("-")[2:]
    mant, exp = h.split("p")
    ip, _, fp = mant.partition(".")
    v = LD(int(ip + fp, 16)) * LD(2) ** LD(int(exp) - 4 * len(fp))
    return -v if neg else v


def load_tables(path=None):
    """D[reverse][class][query base][target base] as long double"""
    D = np.zeros((2, 11, 4, 4), LD)
    for ln in open(path or os.path.join(GOLD, "functions", "damage_dhigh.txt")).read().strip().split("\n"):
        f = ln.split(" ")
        D[1 if f[0] == "rev" else 0, int(f[1])] = np.array([_ld(x) if "p" in x else LD(float(x)) for x in f[2:]], LD).reshape(4, 4)
    return D


class Model:
    def __init__(self, D=None):
        D = load_tables() if D is None else D
        err = LD("0.01")
        seq_err = np.where(np.eye(4, dtype=bool), LD(1) - err, err / LD(3))          # [observed][base], symmetric
        self.logT = np.log(seq_err).astype(np.float64)                                # long double log, stored as double
        # logQ[query class 0..10 | 11 = extended][q][base in query]
        dq = np.maximum(D[0].astype(np.float64), SMOOTH)                              # [class][q][base]
        self.logQ = np.concatenate([np.log(dq), self.logT[None]], 0)
        self.logD = np.log(np.maximum(D.astype(np.float64), SMOOTH))                  # [rev][class][q][target base], double log of a double

    def terms(self, qb, qcls):
        """f, g [n][q][44]: the double addends per forward / reverse record of each slot"""
        tb, l = np.arange(44) // 11, np.arange(44) % 11
        lt = self.logT[tb[None, :], qb[:, None]]                                      # [n][44]   log seqErr.p[tb][qb]
        lq = self.logQ[qcls[:, None], np.arange(4)[None, :], qb[:, None]]             # [n][4]
        b2 = lt[:, None, :] + lq[:, :, None]                                          # [n][4][44]
        ld = self.logD[:, l[None, :], np.arange(4)[:, None], tb[None, :]]             # [2][4][44]
        return b2 + ld[0][None], b2 + ld[1][None]

    def call(self, qb, qiter, qlen, ext, cnt, rev, dtype=LD):
        """answers [n] (uint8), the four sums [n][4] in `dtype` (NaN where the 2/5 rule or coverage <= 1 answered) and `early` [n]."""
        qb, qiter, qlen, ext = (np.asarray(a, np.int64) for a in (qb, qiter, qlen, ext))
        cnt, rev = np.asarray(cnt, np.int64).reshape(-1, 44), np.asarray(rev, np.int64).reshape(-1, 44)
        cov = cnt.reshape(-1, 4, 11).sum(2)
        total = cov.sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            ct, ga = cov[:, 3].astype(np.float64) / total, cov[:, 0].astype(np.float64) / total
        early = (total <= 1) | ((ext == 0) & ((ct >= 0.4) | (ga >= 0.4)))
        qcls = np.where(ext != 0, 11, np.where(qiter < 5, qiter, np.where(qiter >= qlen - 5, 11 - (qlen - qiter), 5)))
        f, g = self.terms(qb, qcls)
        s = np.zeros((len(qb), 4), dtype)
        for slot in range(44):                                                        # ascending slots, the reference's loop order
            c, nr = cnt[:, slot], rev[:, slot]
            if not c.any():
                continue
            have = (c != 0)[:, None]
            s = np.where(have, s + ((c - nr).astype(np.float64)[:, None] * f[:, :, slot]).astype(dtype), s)
            s = np.where(have, s + (nr.astype(np.float64)[:, None] * g[:, :, slot]).astype(dtype), s)
        ans = np.where(early, qb, np.argmax(s, 1)).astype(np.uint8)                   # first maximum wins
        return ans, s, early


def parse_vectors(path):
    """lines `qBase qIter qLen wasCorr 44 counts 44 reverse counts <tab> answer [<tab> kind]` -> (head [n][4], cnt, rev, answers, kinds)"""
    rows = [l.rstrip("\n").split("\t") for l in gzip.open(path, "rt") if l.strip()]
    f = np.array([list(map(int, r[0].split(" "))) for r in rows], np.int64)
    kinds = [r[2] if len(r) > 2 else "" for r in rows]
    return f[:, :4], f[:, 4:48], f[:, 48:92], np.array([int(r[1]) for r in rows], np.uint8), kinds


def device_vectors(head, cnt, rev):
    """the 48 words per pile-up that cdm_debug_call_bases takes: head, then total | reverse << 16 per slot"""
    vec = np.zeros((len(head), 48), np.uint32)
    vec[:, :4] = head
    vec[:, 4:] = cnt | (rev << 16)
    return vec
