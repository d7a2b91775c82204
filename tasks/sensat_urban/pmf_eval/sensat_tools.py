"""read_ply for the point files of SensatUrban: binary little-endian PLY with one `vertex` element of scalar properties
(x y z float, red green blue uchar and, on the labelled splits, class uchar).  Written from the PLY format description
(header lines `format`, `element`, `property <type> <name>`, `end_header`, then the packed records)."""
import numpy as np

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply(filename):
    """-> structured numpy array with one field per vertex property (x, y, z, red, green, blue[, class])"""
    with open(filename, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % filename)
        fmt, count, fields, in_vertex = None, None, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: end_header missing" % filename)
            tok = line.decode("ascii").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "end_header":
                break
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                if count is None and tok[1] != "vertex":
                    raise ValueError("%s: the vertex element must come first" % filename)
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    count = int(tok[2])
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError("%s: list properties on vertices are not supported" % filename)
                fields.append((tok[2], "<" + _PLY_TYPES[tok[1]]))
        if fmt != "binary_little_endian":
            raise ValueError("%s: only binary_little_endian PLY is supported, got %r" % (filename, fmt))
        if count is None or not fields:
            raise ValueError("%s: no vertex element" % filename)
        dtype = np.dtype(fields)
        data = np.frombuffer(f.read(count * dtype.itemsize), dtype=dtype, count=count)
    return data.copy()
