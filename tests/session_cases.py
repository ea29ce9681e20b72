"""The session image's format (m-loam_amd/csrc/session_host.hpp) restated in pure Python / NumPy: a writer, a parser and the checksum, shared by
tests/test_session_cases.py (CPU) and tests/test_gpu_session.py (GPU).

Little-endian. [header: 208 bytes][KEYFRAMES][POINTS][SC][PG], the stored sections back to back, each padded with zero bytes to a multiple of 16.
  header      u32 magic "MLHS", version 1, record sizes 16 / 176 / 376, 4 slots; u64 total bytes, reserved 0; four slots of {u32 kind = slot + 1, u32 0, u64 offset,
              bytes, count, checksum} (all zero: absent); u64 checksum of the 200 bytes before it
  KEYFRAMES   per key: pose[7] f64, cov[36] f64, pos[3] f32, n[3] i32, has_outlier i32, pad i32
  POINTS      float4 {x, y, z, lidar}: key 0 surf, key 0 corner, key 0 outlier, key 1 surf, ...
  SC          head: mlh_sc_opts (64 bytes), i32 n, counter, prefix, last_host_decided, last_skipped, 3 x pad, i64 points_host_decided, points_skipped; then
              descriptors f32, ring keys f32, sector keys f64, column norms f64, positions f64 x 3, has_pos u8 -- each array padded to 16
  PG          i32 count, earliest_loop, max_loops, pad; then 176-byte records {pose[7], last[7], loop_rel[7] f64, i32 loop_index, pad}
checksum of u32 words w_i: sum (w_i XOR 0x9E3779B9) (2 i + 1) mod 2^64."""
import struct

import numpy as np

MAGIC, VERSION, XOR = 0x53484C4D, 1, 0x9E3779B9
HEADER, KEY_BYTES, PG_BYTES, SC_HEAD = 208, 376, 176, 112
KEYFRAMES, POINTS, SC, PG = 0, 1, 2, 3
SC_OPTS = struct.Struct("<diidiiddiid")             # mlh_sc_opts
SC_OPTS_FIELDS = ("lidar_height", "num_ring", "num_sector", "max_radius", "num_exclude_recent", "num_candidates", "search_ratio", "dist_thres",
                  "tree_making_period", "reserved", "loop_distance_threshold")
assert SC_OPTS.size == 64


def checksum(payload) -> int:
    w = np.frombuffer(bytes(payload), "<u4").astype(np.uint64)
    with np.errstate(over="ignore"):
        return int(((w ^ np.uint64(XOR)) * (np.uint64(2) * np.arange(len(w), dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))


def pad16(b: bytes) -> bytes:
    return b + bytes(-len(b) % 16)


def keyframes_payload(keys) -> bytes:
    """keys: dicts with pose (7), cov (36), n (3), has_outlier; pos = float32(pose[:3])"""
    out = b""
    for k in keys:
        out += np.asarray(k["pose"], "<f8").tobytes() + np.asarray(k["cov"], "<f8").reshape(36).tobytes() + np.asarray(k["pose"][:3], "<f4").tobytes()
        out += struct.pack("<5i", *[int(v) for v in k["n"]], int(k["has_outlier"]), 0)
    return pad16(out)


def sc_payload(opts, desc, ring_key, sector_key, col_norm, pos, has_pos, counter, prefix, last, totals) -> bytes:
    """desc (n, S, R) f32 (column-major per entry), ring_key (n, R) f32, sector_key / col_norm (n, S) f64, pos (n, 3) f64, has_pos (n,) u8"""
    n = len(ring_key)
    out = SC_OPTS.pack(*[opts[f] for f in SC_OPTS_FIELDS]) + struct.pack("<8i", n, counter, prefix, last[0], last[1], 0, 0, 0) + struct.pack("<2q", *totals)
    for a, t in ((desc, "<f4"), (ring_key, "<f4"), (sector_key, "<f8"), (col_norm, "<f8"), (pos, "<f8"), (has_pos, "u1")):
        out += pad16(np.ascontiguousarray(a, t).tobytes())
    return out


def pg_payload(records, earliest_loop, max_loops) -> bytes:
    """records: (pose, last, loop_rel, loop_index)"""
    out = struct.pack("<4i", len(records), earliest_loop, max_loops, 0)
    for pose, last, rel, li in records:
        out += np.concatenate([pose, last, rel]).astype("<f8").tobytes() + struct.pack("<2i", li, 0)
    return out


def write(payloads, counts) -> bytes:
    """payloads / counts: per slot (None: absent) -> the image"""
    at, table, body = HEADER, b"", b""
    for k in range(4):
        p = payloads[k]
        if p is None:
            table += bytes(40)
            continue
        assert len(p) % 16 == 0
        table += struct.pack("<2I4Q", k + 1, 0, at, len(p), counts[k], checksum(p))
        body += p
        at += len(p)
    head = struct.pack("<6I2Q", MAGIC, VERSION, 16, PG_BYTES, KEY_BYTES, 4, at, 0) + table
    return head + struct.pack("<Q", checksum(head)) + body


def parse(image) -> dict:
    image = bytes(image)
    magic, version, rp, rg, rk, slots, total, reserved = struct.unpack_from("<6I2Q", image, 0)
    out = dict(magic=magic, version=version, rec_point=rp, rec_pg=rg, rec_key=rk, n_slots=slots, total_bytes=total, reserved=reserved, sections=[],
               header_checksum=struct.unpack_from("<Q", image, 200)[0], header_checksum_computed=checksum(image[:200]))
    for k in range(4):
        kind, res, off, nbytes, count, cs = struct.unpack_from("<2I4Q", image, 40 + 40 * k)
        out["sections"].append(dict(kind=kind, offset=off, bytes=nbytes, count=count, checksum=cs, payload=image[off:off + nbytes] if kind else b""))
    return out


def keys_of(image):
    """the KEYFRAMES records and each key's three clouds out of POINTS"""
    p = parse(image)
    ks, ps = p["sections"][KEYFRAMES], p["sections"][POINTS]
    pts = np.frombuffer(ps["payload"], "<f4").reshape(-1, 4)
    out, at = [], 0
    for i in range(ks["count"]):
        rec = ks["payload"][KEY_BYTES * i:KEY_BYTES * (i + 1)]
        n = struct.unpack_from("<3i", rec, 356)
        clouds = []
        for c in range(3):
            clouds.append(pts[at:at + n[c]])
            at += n[c]
        out.append(dict(pose=np.frombuffer(rec, "<f8", 7), cov=np.frombuffer(rec, "<f8", 36, 56), pos=np.frombuffer(rec, "<f4", 3, 344), n=n,
                        has_outlier=struct.unpack_from("<i", rec, 368)[0], clouds=clouds))
    assert at == ps["count"]
    return out


def small_image() -> bytes:
    """the image tests/host/session_host_main.cpp writes from the same formulae: 2 keyframes (3 + 3 points), 2 SC entries at 2 rings x 3 sectors, 3 pose-graph
    keyframes with one loop edge"""
    keys = []
    for i, (n, ho) in enumerate((((2, 1, 0), 0), ((0, 1, 2), 1))):
        keys.append(dict(pose=[0.5 * j + i for j in range(7)], cov=[1e-4 * (j + 1) + i for j in range(36)], n=n, has_outlier=ho))
    pts = np.array([[j + 0.25, -float(j), 0.5 * j, j % 2] for j in range(6)], "<f4")
    opts = dict(lidar_height=2.0, num_ring=2, num_sector=3, max_radius=80.0, num_exclude_recent=1, num_candidates=4, search_ratio=0.1, dist_thres=0.5,
                tree_making_period=3, reserved=0, loop_distance_threshold=50.0)
    desc = np.arange(12, dtype="<f4") * 0.5
    sc = sc_payload(opts, desc, np.arange(4).reshape(2, 2) * 0.25, np.arange(6) * 1.5, np.arange(6) * 2.5, np.arange(6) - 1.0, [1, 0], 5, 1, (3, 1), (7, 2))
    recs = [([float(i), 1.0, 2.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], [0.1 * i, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], 0 if i == 2 else -1) for i in range(3)]
    return write([keyframes_payload(keys), pts.tobytes(), sc, pg_payload(recs, 0, 128)], [2, 6, 2, 3])


def tile_plan(segments, tile=256):
    """the pack's tiles over clouds given as (arena record, length) in canonical order -> [(src, dst, count)], dst counted from the section's first record"""
    out, dst = [], 0
    for src, n in segments:
        for at in range(0, n, tile):
            out.append((src + at, dst + at, min(tile, n - at)))
        dst += n
    return out
