"""On-disk formats on either side of the hot path.

  SRS file       Params::{write, read}  poly/commitment.rs:241-294
                 u32 k | n x 32 B g (compressed) | n x 32 B g_lagrange (compressed) | u32 len | additional_data
                 The reference decompresses with `from_bytes` under a rayon `parallelize`; here the 2 x n square
                 roots run on the device (h2_dev_points_decompress) and the tables never visit the host as points.
  circuit data   CircuitData::{write, read}  plonk.rs:126-204 + helpers.rs (constraint system, verifying-key commitments,
                 fixed columns, permutation mapping) -- see the section at the end of this file
  witness file   AssignWitnessCollection::{store_witness, fetch_witness}  helpers.rs:920-1015
                 u32 columns | column i at byte offset 4 + (i << (k + 5)): n x 32 B raw (Montgomery) Fr
                 -- consumed by create_proof_from_witness (plonk/prover.rs:916-1500)

  verifier params  ParamsVerifier::{write, read}  poly/commitment.rs:392-433
                 u32 k | u32 public_inputs_size | 32 B g1 | 64 B g2 | 64 B s_g2 | public_inputs_size x 32 B g_lagrange

The G1 point encoding (x little-endian, y parity in bit 7 of byte 31, identity = zeros) is this build's convention:
pairing_bn256@30b052f is not available to check against ("parity unpinned").
The G2 encoding -- the SRS file's additional_data ([s]G2) and the two G2 points of a verifier-params file -- is the same
convention extended to Fq2 = Fq[u] / (u^2 + 1): 64 bytes, x.c0 then x.c1 little-endian, bit 7 of byte 63 = the parity of the
canonical y.c0 (of y.c1 when y.c0 is zero: y and -y always differ in that bit), identity = zeros; equally unpinned.  The
codec is the library's (h2_g2_compress / h2_g2_decompress, pairing.py); decompression also checks the order-r subgroup.
"""
import struct

import numpy as np

from ._lib import check
from .cs_format import _Reader, _u32, cs_fetch, cs_store
from .pairing import g1_limbs, g2_compress, g2_decompress
from .params import Params
from .transcript import _MONT_INV_Q, Q_MOD, point_from_bytes, point_to_bytes
from .verifier import ParamsVerifier


def params_write(device, params, path, additional_data=b""):
    """Params::write.  additional_data: the compressed [s]G2 of the setup (`params_additional_data`; 64 bytes, the G2
    encoding described above) -- what verifier.ParamsVerifier.from_params takes back from `params_read`."""
    torch = device.torch
    with open(path, "wb") as f:
        f.write(struct.pack("<I", params.k))
        for table in (params.g, params.g_lagrange):
            with torch.cuda.stream(device.tstream):
                out = torch.empty((params.n, 32), dtype=torch.uint8, device=device.dev)
            check(device.L.h2_dev_points_compress(table.data_ptr(), params.n, out.data_ptr(), device.stream),
                  "h2_dev_points_compress")
            with torch.cuda.stream(device.tstream):
                f.write(out.cpu().numpy().tobytes())
        f.write(struct.pack("<I", len(additional_data)))
        f.write(additional_data)


def _points_read(device, f, n):
    """the next n compressed points of `f`, decompressed on the device"""
    torch = device.torch
    raw = np.frombuffer(f.read(32 * n), dtype=np.uint8)
    if raw.size != 32 * n:
        raise IOError("truncated params file")
    with torch.cuda.stream(device.tstream):
        d_raw = torch.from_numpy(raw.copy()).to(device.dev)
        pts = torch.empty((n, 8), dtype=torch.int64, device=device.dev)
    check(device.L.h2_dev_points_decompress(d_raw.data_ptr(), n, pts.data_ptr(), device.stream), "h2_dev_points_decompress")
    return pts


def params_read(device, path, k=None, verify=False, seed=None):
    """Params::read -> (Params with both tables resident on the device, additional_data).
    `k` below the file's: the parameters of 2^k rows from the same setup -- only the first 2^k points of g are read and
    decompressed (the g of a smaller k is a prefix), g_lagrange is derived from them (Params.from_powers: the basis is not
    a prefix), the rest of the file is skipped; additional_data ([s]G2) does not depend on k and comes back unchanged.
    `k` above the file's raises ValueError; None or the file's own k reads the file as it is.
    `verify`: the parameters go through Params.assert_valid before they are returned, with the file's additional_data as
    [s]G2 (when it is the 64 bytes of one) and `seed` for the check's randomness: params_check.ParamsError for a file whose
    points, powers or Lagrange basis are wrong.  Off by default -- the reference reads the points as they come."""
    with open(path, "rb") as f:
        (file_k,) = struct.unpack("<I", f.read(4))
        if k is not None and k > file_k:
            raise ValueError("params file %s holds k = %d, cannot give k = %d" % (path, file_k, k))
        if k is not None and k < file_k:
            g = _points_read(device, f, 1 << k)
            f.seek(4 + 64 * (1 << file_k))             # past the rest of g and all of g_lagrange
            additional = _additional_read(f)
            return _checked(device, Params.from_powers(device, k, g), additional, verify, seed), additional
        n = 1 << file_k
        tables = [_points_read(device, f, n) for _ in range(2)]
        (alen,) = struct.unpack("<I", f.read(4))
        additional = f.read(alen)
        if len(additional) != alen:
            raise IOError("truncated params file")
    return _checked(device, Params(device, file_k, tables[0], tables[1]), additional, verify, seed), additional


def _checked(device, params, additional, verify, seed):
    if verify:
        params.assert_valid(device, s_g2=additional if len(additional) == 64 else None, seed=seed)
    return params


def params_additional_data(params):
    """the additional_data `params_write` should carry for a verifier: the compressed [s]G2 of Params.unsafe_setup"""
    return g2_compress(params.s_g2)


def params_verifier_write(pv, path, device=None):
    """ParamsVerifier::write (poly/commitment.rs:392-404).  The Lagrange points are compressed on the host unless they live
    on a device and `device` is given (h2_dev_points_compress)."""
    size = pv.public_inputs_size
    with open(path, "wb") as f:
        f.write(struct.pack("<II", pv.k, size))
        f.write(point_to_bytes(pv.g1) + g2_compress(pv.g2) + g2_compress(pv.s_g2))
        if device is not None and not isinstance(pv.g_lagrange, np.ndarray) and size:
            torch = device.torch
            with torch.cuda.stream(device.tstream):
                out = torch.empty((size, 32), dtype=torch.uint8, device=device.dev)
            check(device.L.h2_dev_points_compress(pv.g_lagrange.data_ptr(), size, out.data_ptr(), device.stream),
                  "h2_dev_points_compress")
            with torch.cuda.stream(device.tstream):
                f.write(out.cpu().numpy().tobytes())
        else:
            raw = np.ascontiguousarray(pv.lagrange_host()[:size], dtype=np.uint64).tobytes()
            for i in range(size):
                x, y = (int.from_bytes(raw[64 * i + 32 * j:64 * i + 32 * j + 32], "little") * _MONT_INV_Q % Q_MOD for j in range(2))
                f.write(point_to_bytes(None if x == 0 and y == 0 else (x, y)))


def params_verifier_read(path, device=None):
    """ParamsVerifier::read (poly/commitment.rs:406-433) -> verifier.ParamsVerifier.  With a `device` the Lagrange points
    are decompressed there and stay resident; without one they are decompressed on the host (public inputs are few) and
    uploaded when a device first commits to them.  IOError / ValueError for a file that is cut short or holds a bad point."""
    with open(path, "rb") as f:
        head = f.read(8 + 32 + 64 + 64)
        if len(head) != 168:
            raise IOError("truncated verifier params file")
        k, size = struct.unpack("<II", head[:8])
        g1, g2, s_g2 = point_from_bytes(head[8:40]), g2_decompress(head[40:104]), g2_decompress(head[104:168])
        if device is not None and size:
            g_lagrange = _points_read(device, f, size)
        else:
            raw = f.read(32 * size)
            if len(raw) != 32 * size:
                raise IOError("truncated verifier params file")
            g_lagrange = np.array([g1_limbs(point_from_bytes(raw[32 * i:32 * i + 32])) for i in range(size)],
                                  dtype=np.uint64).reshape(size, 8)
    return ParamsVerifier(k, s_g2, g_lagrange, size, g1=g1, g2=g2)


def _additional_read(f):
    head = f.read(4)
    if len(head) != 4:
        raise IOError("truncated params file")
    (alen,) = struct.unpack("<I", head)
    additional = f.read(alen)
    if len(additional) != alen:
        raise IOError("truncated params file")
    return additional


def witness_store(path, k, columns):
    """store_witness: columns = (n, 4) u64 arrays in the in-memory (Montgomery) representation"""
    n = 1 << k
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(columns)))
        for col in columns:
            col = np.ascontiguousarray(col, dtype=np.uint64)
            assert col.shape == (n, 4)
            f.write(col.tobytes())


def witness_fetch(path, k):
    """fetch_witness: the columns as read-only memory maps of the file (bundle size 2^(k+5) bytes)"""
    n = 1 << k
    with open(path, "rb") as f:
        (count,) = struct.unpack("<I", f.read(4))
    return [np.memmap(path, dtype=np.uint64, mode="r", offset=4 + (i << (k + 5)), shape=(n, 4)) for i in range(count)]


# ---- CircuitData (plonk.rs:126-204; helpers.rs:64-112,237-758,902-917) ---------------------------------------------
#   u32 j (quotient degree + 1 = cs.degree()) | u32 k | constraint system (write_cs, helpers.rs:406-456) |
#   fixed commitments, permutation commitments (32 B compressed each, plonk.rs:60-67) |
#   fixed columns: u32 count, each u32 n + n x 32 B raw (Montgomery) Fr (helpers.rs:182-199, 237-253) |
#   permutation mapping: u32 columns, u32 length per column, then (u32 column, u32 row) pairs (helpers.rs:114-179)
# Every integer is a little-endian u32 (the constraint system's own encoding: cs_format.py).
def circuit_data_write(path, device, params, pk):
    """CircuitData::write for a key made by prover.keygen"""
    cs, n = pk.cs, params.n
    with open(path, "wb") as f:
        f.write(_u32(cs.degree()) + _u32(params.k))
        f.write(cs_store(cs))
        for P in list(pk.fixed_commitments) + list(pk.perm_commitments):
            f.write(point_to_bytes(P))
        f.write(_u32(len(pk.fixed_values)))
        for t in pk.fixed_values:
            f.write(_u32(n))
            f.write(np.ascontiguousarray(device.download(t)).tobytes())
        map_col, map_row = pk.mapping
        f.write(_u32(len(map_col)))
        for col in map_col:
            f.write(_u32(len(col)))
        for mc, mr in zip(map_col, map_row):
            f.write(np.stack([mc, mr], axis=1).astype("<u4").tobytes())


def circuit_data_read(path, name="circuit"):
    """CircuitData::read -> dict(j, k, cs, fixed_commitments, perm_commitments (compressed bytes), fixed (Montgomery
    (n, 4) u64 columns), mapping (map_col, map_row)); `prover.keygen_from_info` turns it into a proving key
    (CircuitData::into_proving_key, plonk.rs:196-198)"""
    with open(path, "rb") as f:
        r = _Reader(f.read())
    j, k = r.u32(), r.u32()
    cs = cs_fetch(r, name)
    cs.set_minimum_degree(j)     # the domain the key was made for (a `set_minimum_degree` call is not part of the stream)
    try:
        fits = cs.degree() == j
    except AssertionError:
        fits = False
    if not fits:
        raise IOError("circuit data: the constraint system does not fit a domain of degree %d" % j)
    fixed_commitments = [bytes(r.take(32)) for _ in range(cs.num_fixed)]
    perm_commitments = [bytes(r.take(32)) for _ in range(len(cs.perm_columns))]
    fixed = []
    for _ in range(r.u32()):
        m = r.u32()
        fixed.append(np.frombuffer(r.take(32 * m), dtype=np.uint64).reshape(m, 4))
    lengths = [r.u32() for _ in range(r.u32())]
    map_col, map_row = [], []
    for m in lengths:
        pairs = np.frombuffer(r.take(8 * m), dtype="<u4").reshape(m, 2)
        map_col.append(np.ascontiguousarray(pairs[:, 0]))
        map_row.append(np.ascontiguousarray(pairs[:, 1]))
    return {"j": j, "k": k, "cs": cs, "fixed_commitments": fixed_commitments, "perm_commitments": perm_commitments,
            "fixed": fixed, "mapping": (map_col, map_row)}
