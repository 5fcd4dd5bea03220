"""Row-loop references for the text operators (otbx_text_pred, text gather).

Two independent LIKE matchers, each for both encodings:
  like_rec — the reference's recursive MatchText (like_match.c:78) restated
             statement by statement over the raw pattern bytes, with its
             TRUE / FALSE / ABORT results.
  like_dp  — a dynamic-programming table over (text position, pattern
             token): no recursion, no restart logic, no normalisation of
             wildcard runs. Character steps come from the NextChar rule.
Comparisons are Python bytes comparisons (memcmp over the common prefix,
unsigned, then the shorter is smaller). The gather reference is list
indexing.
"""

LIKE_TRUE, LIKE_FALSE, LIKE_ABORT = 1, 0, -1


class TrailingEscape(ValueError):
    """LIKE pattern must not end with escape character"""


def next_char(t, i, utf8):
    """NextChar (like.c:142): one byte, then every continuation byte that
    is still inside the text; one byte in a single-byte encoding."""
    i += 1
    if utf8:
        while i < len(t) and (t[i] & 0xC0) == 0x80:
            i += 1
    return i


# ---- (a) the recursion ----

def _match_text(t, ti, p, pi, utf8):
    tlen, plen = len(t), len(p)
    if plen - pi == 1 and p[pi] == 0x25:
        return LIKE_TRUE
    while ti < tlen and pi < plen:
        if p[pi] == 0x5C:                     # backslash
            pi += 1
            if pi >= plen:
                raise TrailingEscape()
            if p[pi] != t[ti]:
                return LIKE_FALSE
        elif p[pi] == 0x25:                   # %
            pi += 1
            while pi < plen:
                if p[pi] == 0x25:
                    pi += 1
                elif p[pi] == 0x5F:
                    if ti >= tlen:
                        return LIKE_ABORT
                    ti = next_char(t, ti, utf8)
                    pi += 1
                else:
                    break
            if pi >= plen:
                return LIKE_TRUE
            if p[pi] == 0x5C:
                if plen - pi < 2:
                    raise TrailingEscape()
                firstpat = p[pi + 1]
            else:
                firstpat = p[pi]
            while ti < tlen:
                if t[ti] == firstpat:
                    m = _match_text(t, ti, p, pi, utf8)
                    if m != LIKE_FALSE:
                        return m
                ti = next_char(t, ti, utf8)
            return LIKE_ABORT
        elif p[pi] == 0x5F:                   # _
            ti = next_char(t, ti, utf8)
            pi += 1
            continue
        elif p[pi] != t[ti]:
            return LIKE_FALSE
        ti += 1
        pi += 1
    if ti < tlen:
        return LIKE_FALSE
    while pi < plen and p[pi] == 0x25:
        pi += 1
    if pi >= plen:
        return LIKE_TRUE
    return LIKE_ABORT


def like_rec(text, pattern, utf8=True):
    return _match_text(bytes(text), 0, bytes(pattern), 0, utf8) == LIKE_TRUE


# ---- (b) the table ----

LIT, ANY, SEQ = 0, 1, 2


def tokens(pattern):
    """pattern bytes → [(kind, byte)]; a trailing lone escape is refused."""
    out = []
    i = 0
    while i < len(pattern):
        c = pattern[i]
        if c == 0x25:
            out.append((SEQ, 0))
        elif c == 0x5F:
            out.append((ANY, 0))
        else:
            if c == 0x5C:
                i += 1
                if i >= len(pattern):
                    raise TrailingEscape()
                c = pattern[i]
            out.append((LIT, c))
        i += 1
    return out


def like_dp(text, pattern, utf8=True):
    t = bytes(text)
    tok = tokens(bytes(pattern))
    n, m = len(t), len(tok)
    nxt = [next_char(t, i, utf8) for i in range(n)]
    # ok[i][k]: tokens k.. match text i..
    ok = [[False] * (m + 1) for _ in range(n + 1)]
    for i in range(n, -1, -1):
        for k in range(m, -1, -1):
            if k == m:
                v = i == n
            else:
                kind, b = tok[k]
                if kind == LIT:
                    v = i < n and t[i] == b and ok[i + 1][k + 1]
                elif kind == ANY:
                    v = i < n and ok[nxt[i]][k + 1]
                else:
                    v = ok[i][k + 1] or (i < n and ok[nxt[i]][k])
            ok[i][k] = v
    return ok[0][0]


def has_trailing_escape(pattern):
    p = bytes(pattern)
    return (len(p) - len(p.rstrip(b"\\"))) % 2 == 1


# ---- predicates over a column ----

CMP = {"=": lambda a, b: a == b, "<>": lambda a, b: a != b,
       "<": lambda a, b: a < b, "<=": lambda a, b: a <= b,
       ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}
OPS = ("like", "not like") + tuple(CMP)


def ref_pred(rows, op, rhs, utf8=True, matcher=like_dp):
    """rows: list of bytes / None. rhs: bytes, or a list of bytes / None of
    the same length. → (values, nulls) as lists of 0 / 1; the value under a
    NULL is 0."""
    if isinstance(rhs, str):
        rhs = rhs.encode("utf-8")
    vals, nulls = [], []
    for i, a in enumerate(rows):
        b = rhs[i] if isinstance(rhs, list) else rhs
        if a is None or b is None:
            vals.append(0)
            nulls.append(1)
            continue
        if op == "like":
            v = matcher(a, b, utf8)
        elif op == "not like":
            v = not matcher(a, b, utf8)
        else:
            v = CMP[op](a, b)
        vals.append(1 if v else 0)
        nulls.append(0)
    return vals, nulls


def clamped_rows(raw, offs, nulls=None):
    """the rows of (bytes, offs) under the kernels' clamping policy"""
    nb = len(raw)
    out = []
    for i in range(len(offs) - 1):
        if nulls is not None and nulls[i]:
            out.append(None)
            continue
        s = min(max(int(offs[i]), 0), nb)
        e = min(max(int(offs[i + 1]), 0), nb)
        out.append(bytes(raw[s:e]) if e > s else b"")
    return out


def ref_gather(rows, perm):
    n = len(rows)
    return [rows[min(max(int(j), 0), n - 1)] for j in perm]


# the 92 words TPC-H builds P_NAME from (specification 4.2.3, "colors")
P_NAME_WORDS = (
    "almond antique aquamarine azure beige bisque black blanched blue blush "
    "brown burlywood burnished chartreuse chiffon chocolate coral cornflower "
    "cornsilk cream cyan dark deep dim dodger drab firebrick floral forest "
    "frosted gainsboro ghost goldenrod green grey honeydew hot indian ivory "
    "khaki lace lavender lawn lemon light lime linen magenta maroon medium "
    "metallic midnight mint misty moccasin navajo navy olive orange orchid "
    "pale papaya peach peru pink plum powder puff purple red rose rosy royal "
    "saddle salmon sandy seashell sienna sky slate smoke snow spring steel "
    "tan thistle tomato turquoise violet wheat white yellow").split()
