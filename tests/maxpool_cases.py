"""Shared by the tiled max-pool tests (tests/test_gpu_maxpool_tiles.py and the CPU half
tests/test_maxpool_tiles_host.py): the constants of csrc/maxpool.hip read out of its text, a model of the loops of
gnm_maxpool_tile_fwd_kernel / gnm_maxpool_tile_bwd_kernel, the graph and feature builders and the two case tables.
No tests here.

The tiled kernels run one workgroup per graph.  With LPR = F / 4 lanes per row a wave holds RPW = 64 / LPR rows, the 16
waves of the workgroup cover 16 RPW rows a pass, and a row's candidate ids are fetched LPR at a time, kMaxTileAhead
chunks ahead of the chunk being consumed: the prologue fetches chunks 0 .. kMaxTileAhead - 1 and the in-loop refill
fetches a real id only for a row with more than kMaxTileAhead * LPR candidates.  tests/test_gpu_maxpool.py stays short
of that (and of a second pass, the unrolled staging loop and the LDS limits) everywhere but in one 400-node
comparison; TILE_CASES walks through those states for F = 64 and F = 32, on the forward's lists ("out") and on the
backward's ("in", the transposed graph)."""
import collections
import functools
import re
import zlib

import numpy as np

Consts = collections.namedtuple("Consts", "threads ahead colmin_rows lds_budget")
CONSTS = Consts(1024, 4, 256, 160 * 1024)          # what the tables are built on; the host test holds the source to it


def tile_constants(src, common_src):
    """Consts read out of the text of csrc/maxpool.hip and csrc/gnm_common.h"""
    def find(text, name, where):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*(?:\*\s*(\d+)\s*)?;" % name, text)
        assert m, "%s: `constexpr int %s = <value>;` not found: the tiled max-pool tables " \
                  "(tests/maxpool_cases.py TILE_CASES / COLMIN_CASES) are built on it and have to be revisited" % (where, name)
        return int(m.group(1)) * (int(m.group(2)) if m.group(2) else 1)
    return Consts(find(src, "kMaxTileThreads", "csrc/maxpool.hip"), find(src, "kMaxTileAhead", "csrc/maxpool.hip"),
                  find(src, "kColminRows", "csrc/maxpool.hip"), find(common_src, "kLdsBudget", "csrc/gnm_common.h"))


# --------------------------------------------------------------------------- the model of the kernel loops
def lds_bytes(F, n_max, which):
    """dynamic LDS of one workgroup: n_max + 1 rows (the last is what empty slots read) of fp32 values -- the backward
    adds a 16-bit selected row per element -- and n_max + 1 list offsets"""
    per_row = {"fwd": 4 * F + 4, "bwd": 6 * F + 4}[which]
    return (n_max + 1) * per_row


def lds_fits(F, n_max, which, consts=CONSTS):
    return lds_bytes(F, n_max, which) <= consts.lds_budget


def lds_limit(F, which, consts=CONSTS):
    """the largest n_max the tiled kernel takes"""
    return consts.lds_budget // lds_bytes(F, 0, which) - 1


TilePlan = collections.namedtuple("TilePlan", "passes unrolled offs_trips invalid_slots wave_trips refill_rows mixed_wave "
                                              "refill_sizes last_chunks")


def tile_plan(F, degs, consts=CONSTS):
    """What one workgroup of a tiled kernel does on a graph whose rows have `degs` candidates in their lists (the
    forward: out-degrees; the backward: distinct in-degrees, plus the node itself in the self-loop form):
      passes         trips of the row loop of wave 0 (16 waves x RPW rows a pass)
      unrolled       the 4-deep unrolled staging loop of the forward runs
      offs_trips     trips of the loop that stages the n + 1 list offsets
      invalid_slots  slots of the last wave that hold no row
      wave_trips     per wave (RPW consecutive rows) the trips of the candidate loop, max ceil(deg / LPR)
      refill_rows    rows whose in-loop refill fetches a real id (deg > kMaxTileAhead * LPR)
      mixed_wave     some wave holds a row without candidates and a refilling row
      refill_sizes   the set of real-id counts (1 .. LPR) of the in-loop refills
      last_chunks    the set of id counts (1 .. LPR) of the rows' last chunks"""
    assert F % 4 == 0 and 64 % (F // 4) == 0
    LPR = F // 4
    RPW = 64 // LPR
    n = len(degs)
    waves = consts.threads // 64
    wave_trips, mixed = [], False
    refill_sizes, last_chunks = set(), set()
    for r0 in range(0, n, RPW):
        group = [int(d) for d in degs[r0:r0 + RPW]]
        wave_trips.append(max(-(-d // LPR) for d in group))
        mixed = mixed or (min(group) == 0 and max(group) > consts.ahead * LPR)
    for d in degs:
        d = int(d)
        if d:
            last_chunks.add(d - (-(-d // LPR) - 1) * LPR)
        for e0 in range(0, d, LPR):                                       # the row's own trips of the candidate loop
            got = min(LPR, max(0, d - (e0 + consts.ahead * LPR)))
            if got:
                refill_sizes.add(got)
    return TilePlan(passes=-(-n // (waves * RPW)), unrolled=n * LPR > 3 * consts.threads,
                    offs_trips=-(-(n + 1) // consts.threads), invalid_slots=(-n) % RPW, wave_trips=wave_trips,
                    refill_rows=sum(1 for d in degs if d > consts.ahead * LPR), mixed_wave=mixed,
                    refill_sizes=refill_sizes, last_chunks=last_chunks)


def fwd_degs(graph):
    return [len(x) for x in graph.neighbors]


def bwd_degs(graph, self_last):
    """lengths of the backward's lists: for every node the DISTINCT rows that list it, and itself in the self-loop form"""
    n = len(graph.g)
    pairs = {(j, i) for i, nb in enumerate(graph.neighbors) for j in nb}
    if self_last:
        pairs |= {(j, j) for j in range(n)}
    deg = [0] * n
    for j, _ in pairs:
        deg[j] += 1
    return deg


# --------------------------------------------------------------------------- graphs
class Graph:
    """what gnm.maxnb.MaxNeighbours and oracle.gin_oracle.build_padded_neighbors read of an S2VGraph"""

    def __init__(self, neighbors):
        self.g = range(len(neighbors))
        self.num_nodes = len(neighbors)
        self.neighbors = neighbors
        self.max_neighbor = max((len(x) for x in neighbors), default=0)


LADDER_LEN = 13                                    # coprime to RPW (4 and 8): every wave mixes degrees


def ladder(LPR, n):
    steps = [0, 1, LPR - 1, LPR, LPR + 1, 4 * LPR - 1, 4 * LPR, 4 * LPR + 1, 5 * LPR - 1, 5 * LPR, 5 * LPR + 1, 8 * LPR + 1,
             min(n - 1, 400)]
    assert len(steps) == LADDER_LEN
    return [max(0, min(d, n - 1)) for d in steps]


def out_lists(rng, LPR, n):
    """row r lists ladder[r % 13] distinct other nodes in random order, node 0 among them (a hub of in-degree ~ n)"""
    lad = ladder(LPR, n)
    nb = []
    for r in range(n):
        d = lad[r % LADDER_LEN]
        if d == 0:
            nb.append([])
            continue
        pool = np.delete(np.arange(1, n), r - 1)                          # neither the hub nor the row itself
        row = np.concatenate([rng.permutation(pool)[:d - 1], [0]])
        nb.append([int(x) for x in rng.permutation(row)])
    return nb


def regular_lists(rng, LPR, n):
    d = 4 * LPR + 1                                                       # every row refills exactly one id
    assert d <= n - 1
    return [[int(x) for x in rng.permutation(np.delete(np.arange(n), r))[:d]] for r in range(n)]


def transposed_lists(rng, nb):
    t = [[] for _ in nb]
    for i, row in enumerate(nb):
        for j in row:
            t[j].append(i)
    return [[int(x) for x in rng.permutation(row)] if row else [] for row in t]


def add_repeats(nb, donor):
    """row 0 repeats two neighbours and lists itself (a row too short for that borrows two of `donor`'s first)"""
    row = list(nb[0])
    if len(row) < 2:
        row = row + [x for x in donor if x not in row][:2 - len(row)]
    nb[0] = row + row[:2] + [0]


TileCase = collections.namedtuple("TileCase", "F sizes kind feat")


def case_id(case):
    return "F%d-%s-n%s-%s" % (case.F, case.kind, "_".join(map(str, case.sizes)), case.feat)


@functools.lru_cache(maxsize=4)
def build_graphs(F, sizes, kind):
    """the graphs of a case (they do not depend on its feature kind)"""
    rng = np.random.default_rng(zlib.crc32(("%d %s %s" % (F, sizes, kind)).encode()))
    LPR = F // 4
    graphs = []
    for k, n in enumerate(sizes):
        if kind == "regular":
            nb = regular_lists(rng, LPR, n)
        else:
            nb = out_lists(rng, LPR, n)
            donor = nb[2] if n > 2 else []
            if kind == "in":
                nb = transposed_lists(rng, nb)
                donor = nb[1] if n > 2 else []
            else:
                assert kind == "out", kind
            if len(sizes) > 1 and k == 0:
                add_repeats(nb, donor)
        graphs.append(Graph(nb))
    return graphs


def case_graphs(case):
    return build_graphs(case.F, tuple(case.sizes), case.kind)


def node_offsets(graphs):
    return np.concatenate([[0], np.cumsum([g.num_nodes for g in graphs])]).astype(np.int64)


def coarse(rng, N, F):
    """integers -2 .. 2, the zeros randomly signed: ties everywhere, and -0.0 == 0.0 ties between different bits"""
    h = rng.integers(-2, 3, (N, F)).astype(np.float32)
    h[(h == 0) & (rng.random((N, F)) < 0.5)] = np.float32(-0.0)
    return h


def nan_columns(F):
    return [c for c in range(F) if c % 4 == 1]


def case_features(case, graphs):
    F = case.F
    LPR = F // 4
    off = node_offsets(graphs)
    N = int(off[-1])
    rng = np.random.default_rng(zlib.crc32(case_id(case).encode()))
    if case.feat == "relu":                              # what the layers above 0 see: many exact zeros
        return np.maximum(rng.standard_normal((N, F)), 0).astype(np.float32)
    h = coarse(rng, N, F)
    if case.feat == "coarse":
        return h
    if case.feat == "nan":
        cols = nan_columns(F)
        # columns 1 and 5 hold one NaN each: a long row's first neighbour, and a neighbour past position 4 LPR of a list
        # (the first id its in-loop refill fetches; the last of its list where no list is that long)
        hubs = set(int(x) for x in off[:-1])
        rows = sorted(((len(nb), int(off[k]) + i, [int(off[k]) + j for j in nb]) for k, g in enumerate(graphs)
                       for i, nb in enumerate(g.neighbors) if nb), key=lambda t: (-t[0], t[1]))
        first = next(t for t in rows if t[2][0] not in hubs)
        h[first[2][0], cols[0]] = np.nan
        late = next(t for t in rows if t[1] != first[1] and t[2][min(4 * LPR, t[0] - 1)] not in hubs)
        h[late[2][min(4 * LPR, late[0] - 1)], cols[1]] = np.nan
        k = max(1, N // 7)
        h[rng.integers(0, N, k), rng.choice(cols[2:], k)] = np.nan
        return h
    if case.feat == "ninf":
        k = max(1, N // 9)
        h[rng.integers(0, N, k), rng.integers(0, F, k)] = np.inf
        h[rng.choice(N, max(1, min(3, N // 20)), replace=False), :] = -np.inf
        h[:, 2] = -np.inf
        return h
    raise ValueError(case.feat)


ALL_FEATS = ("relu", "coarse", "nan", "ninf")
TWO_FEATS = ("relu", "coarse")


def _tile_cases():
    table = {64: dict(out=[63, 64, 65, 193, 421, 422, 629, 630], inn=[65, 421], ragged=[65, 1, 2, 129, 64, 400, 3],
                      regular=130, all_feats=65),
             32: dict(out=[127, 128, 129, 385, 834, 835, 1024, 1240, 1241], inn=[129, 834],
                      ragged=[129, 1, 2, 257, 128, 400, 9], regular=70, all_feats=129)}
    cases = []
    for F, t in table.items():
        for kind, ns in (("out", t["out"]), ("in", t["inn"])):
            for n in ns:
                cases += [TileCase(F, (n,), kind, f) for f in (ALL_FEATS if n == t["all_feats"] else TWO_FEATS)]
        for kind in ("out", "in"):
            cases += [TileCase(F, tuple(t["ragged"]), kind, f) for f in ALL_FEATS]
        cases += [TileCase(F, (t["regular"],), "regular", f) for f in TWO_FEATS]
    return cases


TILE_CASES = _tile_cases()
EPS = 0.37                                         # learn_eps True; learn_eps False is the self-loop form, no eps


# --------------------------------------------------------------------------- the column minimum
ColminCase = collections.namedtuple("ColminCase", "N F variant")
COLMIN_SMALL = [(N, F) for N in (1, 2, 5, 29, 33, 255, 256, 257, 513) for F in (1, 7, 64, 65)] + [(1000, 130), (800, 400)]
COLMIN_LARGE = [(28672, 3), (28673, 3), (32768, 65), (61700, 7)]
COLMIN_VARIANTS = ("plain", "first", "last", "tie", "nan2")
COLMIN_ONEHOT = (800, 400)
COLMIN_CASES = [ColminCase(N, F, v) for N, F in COLMIN_SMALL + COLMIN_LARGE for v in COLMIN_VARIANTS]


def colmin_blocks(N, consts=CONSTS):
    return -(-N // consts.colmin_rows)


def colmin_nan_rows(N, consts=CONSTS):
    """(r1, r2), r1 < r2: the rows of the two NaNs.  Where the table allows they sit in different blocks of the partial
    pass and the later one has the smaller phase: of the final pass (block % 16) from 17 blocks on, and of the partial
    pass (row % 4) always"""
    R, nblk = consts.colmin_rows, colmin_blocks(N, consts)
    if nblk >= 17:
        return 5 * R + 3, 16 * R
    if N > R:
        return 3, R
    if N >= 5:
        return 3, 4
    return 0, N - 1


def colmin_tie_rows(N, consts=CONSTS):
    """(r1, r2), r1 <= r2: two rows holding the same minimum, in block 0 and in the last block of the partial pass"""
    last0 = (colmin_blocks(N, consts) - 1) * consts.colmin_rows
    return min(N - 1, 1), min(N - 1, last0 + 2)


def colmin_input(case, consts=CONSTS):
    N, F = case.N, case.F
    rng = np.random.default_rng(zlib.crc32(("colmin %d %d %s" % case).encode()))
    if (N, F) == COLMIN_ONEHOT:
        h = np.eye(F, dtype=np.float32)[rng.integers(0, F, N)]
    else:
        h = coarse(rng, N, F)
    low = np.float32(-5)                                                  # below everything else
    if case.variant == "first":
        h[0, :] = low
    elif case.variant == "last":
        h[N - 1, :] = low
    elif case.variant == "tie":                                           # a row of block 0 and a row of the last block
        for r in colmin_tie_rows(N, consts):
            h[r, :] = low
    elif case.variant == "nan2":
        r1, r2 = colmin_nan_rows(N, consts)
        h[r1, ::3] = np.nan
        h[r2, ::3] = np.nan
    else:
        assert case.variant == "plain"
    return h
