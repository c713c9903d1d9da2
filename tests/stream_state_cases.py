"""Named stream-state blobs for stream_state_validate (liodom_amd/csrc/stream_state_format.h), defined once: the host program of
test_stream_state_format.py judges each, test_gpu_stream_state_refusals.py offers the refusals to liodom_import_stream_state.

cases(good, taker) derives them from a good blob and the handle that is to take it, taker = Taker(fingerprint, mapping, edge_cap,
recv_cap), and yields Case(name, blob, taker, code): `blob` offered to `taker` (the given one, or one with other capacities where
the case is about those) returns `code`.  What a good blob cannot show is left out: the received-map cases need a mapping blob with
n_recv > 0, the padding case a local_map_size that is no multiple of 4, the j = 1 / j = 3 order cases four frames.  Pure Python."""
import collections
import struct

OK, INVALID_ARG, CAPACITY = 0, -1, -3
INT32_MAX = 2 ** 31 - 1
Taker = collections.namedtuple("Taker", "fingerprint mapping edge_cap recv_cap")      # fingerprint: the six header words, in order
Case = collections.namedtuple("Case", "name blob taker code")

# byte offsets (stream_state_format.h): header, then the record's int32 fields behind its 43 doubles, then the counts
VERSION, HEADER_BYTES, TOTAL, FINGERPRINT = 8, 12, 16, 24
ODOM = 64
INITIALIZED, APPEND_RAW, FRAME_COUNT, N_FRAMES, SCAN_COUNTER, STATUS, N_POINTS, N_RECV = (64 + 344 + 4 * i for i in range(8))
COUNTS = 480
FP_NAMES = ("local_map_size", "mapping", "filter_local_map", "use_imu", "pose_rotation_mode", "lm_apply_step_on_ftol")


def put(blob, off, fmt, *values):
    b = bytearray(blob)
    struct.pack_into(fmt, b, off, *values)
    return bytes(b)


def get(blob, off, fmt="<i"):
    return struct.unpack_from(fmt, blob, off)[0]


def fingerprint_of(blob):
    return tuple(struct.unpack_from("<6I", blob, FINGERPRINT))


def counts_of(blob):
    P = get(blob, FINGERPRINT, "<I")
    return list(struct.unpack_from("<%di" % ((P + 3) // 4 * 4), blob, COUNTS))


def with_counts(blob, counts):
    return put(blob, COUNTS, "<%di" % len(counts), *counts)


def rebuilt(blob, n_frames, n_recv):
    """The blob of the same stream with its first n_frames frames only (frame_count = scan_counter = n_frames) and the first n_recv
    points of its received map: consistent in every size."""
    counts = counts_of(blob)
    pts_off = COUNTS + 4 * len(counts)
    old_points = get(blob, N_POINTS)
    counts = counts[:n_frames] + [0] * (len(counts) - n_frames)
    n_points = sum(counts)
    pts = blob[pts_off:pts_off + 16 * n_points] + blob[pts_off + 16 * old_points:pts_off + 16 * (old_points + n_recv)]
    b = with_counts(blob[:pts_off], counts) + pts
    for off, v in ((FRAME_COUNT, n_frames), (N_FRAMES, n_frames), (SCAN_COUNTER, n_frames), (N_POINTS, n_points), (N_RECV, n_recv)):
        b = put(b, off, "<i", v)
    return put(b, TOTAL, "<Q", len(b))


def cases(good, taker):
    P, fc, nf, n_points, n_recv = (get(good, off) for off in (FINGERPRINT, FRAME_COUNT, N_FRAMES, N_POINTS, N_RECV))
    cnt = counts_of(good)
    pts_off = COUNTS + 4 * len(cnt)
    big = max(range(len(cnt)), key=lambda j: cnt[j])                    # a frame with points: one can be taken away
    assert fingerprint_of(good) == taker.fingerprint and nf >= 2 and cnt[big] >= 1 and max(cnt) <= taker.edge_cap and n_recv <= taker.recv_cap

    def case(name, blob, code, **other):
        return Case(name, bytes(blob), taker._replace(**other), code)

    # ---- accepted ----
    yield case("the good blob", good, OK)
    yield case("larger capacities", good, OK, edge_cap=taker.edge_cap + 100, recv_cap=taker.recv_cap + 100)
    never = put(put(rebuilt(good, 0, 0), INITIALIZED, "<i", 0), STATUS, "<I", 0)
    yield case("a stream that never ran", never, OK)
    yield case("a count equal to edge_cap", good, OK, edge_cap=max(cnt))
    yield case("NaN in odom", put(good, ODOM + 8 * 3, "<d", float("nan")), OK)
    yield case("any status bits", put(good, STATUS, "<I", 0xFFFFFFFF), OK)
    # ---- no blob of this handle ----
    for n in (0, 63, 64, 479, 480, pts_off - 1):
        yield case("length %d" % n if n != pts_off - 1 else "length points_offset - 1", good[:n], INVALID_ARG)
    yield case("the blob plus 16 bytes", good + b"\0" * 16, INVALID_ARG)
    yield case("magic with a flipped bit", bytes([good[0] ^ 1]) + good[1:], INVALID_ARG)
    yield case("magic LIODOMMP", b"LIODOMMP" + good[8:], INVALID_ARG)
    yield case("version 2", put(good, VERSION, "<I", 2), INVALID_ARG)
    yield case("header_bytes 65", put(good, HEADER_BYTES, "<I", 65), INVALID_ARG)
    yield case("total_bytes + 16", put(good, TOTAL, "<Q", len(good) + 16), INVALID_ARG)
    yield case("total_bytes - 16", put(good, TOTAL, "<Q", len(good) - 16), INVALID_ARG)
    for i, name in enumerate(FP_NAMES):
        yield case("another " + name, put(good, FINGERPRINT + 4 * i, "<I", taker.fingerprint[i] + 1), INVALID_ARG)
    # ---- the record ----
    yield case("frame_count -1", put(good, FRAME_COUNT, "<i", -1), INVALID_ARG)
    yield case("n_frames one short", put(good, N_FRAMES, "<i", nf - 1), INVALID_ARG)          # (P = 5, frame_count 7: 4 and 6)
    yield case("n_frames one long", put(good, N_FRAMES, "<i", nf + 1), INVALID_ARG)
    yield case("frame_count below n_frames", put(put(good, FRAME_COUNT, "<i", nf - 2), SCAN_COUNTER, "<i", nf - 2), INVALID_ARG)
    yield case("scan_counter is not frame_count", put(good, SCAN_COUNTER, "<i", fc + 1), INVALID_ARG)
    yield case("n_points -1", put(good, N_POINTS, "<i", -1), INVALID_ARG)
    yield case("n_recv -1", put(good, N_RECV, "<i", -1), INVALID_ARG)
    if not taker.mapping and n_recv == 0:
        one = put(put(good + b"\0" * 16, N_RECV, "<i", 1), TOTAL, "<Q", len(good) + 16)
        yield case("n_recv 1, sizes consistent, mapping off", one, INVALID_ARG)
    yield case("initialized 2", put(good, INITIALIZED, "<i", 2), INVALID_ARG)
    yield case("initialized -1", put(good, INITIALIZED, "<i", -1), INVALID_ARG)
    yield case("append_raw 2", put(good, APPEND_RAW, "<i", 2), INVALID_ARG)
    yield case("n_points + 1, total_bytes unchanged", put(good, N_POINTS, "<i", n_points + 1), INVALID_ARG)
    yield case("n_points - 1, total_bytes unchanged", put(good, N_POINTS, "<i", n_points - 1), INVALID_ARG)
    yield case("n_points and n_recv INT32_MAX", put(put(good, N_POINTS, "<i", INT32_MAX), N_RECV, "<i", INT32_MAX), INVALID_ARG)
    # ---- the counts ----
    yield case("a negative count, the sum kept", with_counts(good, [-1, cnt[1] + cnt[0] + 1] + cnt[2:]), INVALID_ARG)
    less = [c - (i == big) for i, c in enumerate(cnt)]                  # one point fewer
    if len(cnt) > P:
        yield case("a count in a padding entry, the sum kept", with_counts(good, less[:P] + [1] + less[P + 1:]), INVALID_ARG)
    short = good if nf < P else rebuilt(good, P - 2, n_recv)
    s_cnt, s_nf = counts_of(short), get(short, N_FRAMES)
    s_big = max(range(len(s_cnt)), key=lambda j: s_cnt[j])
    assert s_nf < P and s_cnt[s_big] >= 1
    yield case("a count behind n_frames, the sum kept", with_counts(short, [1 if i == s_nf else c - (i == s_big) for i, c in enumerate(s_cnt)]), INVALID_ARG)
    yield case("counts sum to n_points - 1", with_counts(good, less), INVALID_ARG)
    # ---- capacities, and which rule wins ----
    yield case("edge_cap one below the largest count", good, CAPACITY, edge_cap=max(cnt) - 1)
    if nf >= 4:
        over = taker.edge_cap + 1
        yield case("count 1 above edge_cap, count 3 negative", with_counts(good, [over if j == 1 else -1 if j == 3 else c for j, c in enumerate(cnt)]), CAPACITY)
        yield case("count 1 negative, count 3 above edge_cap", with_counts(good, [-1 if j == 1 else over if j == 3 else c for j, c in enumerate(cnt)]), INVALID_ARG)
    yield case("a count above edge_cap and a wrong sum", with_counts(good, [taker.edge_cap + 1] + cnt[1:]), CAPACITY)
    if taker.mapping and n_recv > 0:
        yield case("n_recv equal to recv_cap", good, OK, recv_cap=n_recv)
        yield case("recv_cap one below n_recv", good, CAPACITY, recv_cap=n_recv - 1)
        yield case("n_recv above recv_cap and a wrong sum", with_counts(good, less), INVALID_ARG, recv_cap=n_recv - 1)
