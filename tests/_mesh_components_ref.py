"""The yardstick of the mesh-component kernels: include/tinynerf_hip.h's definition restated with a plain sequential
union-find -- labels, face counts, stats, and the filter with src.  numpy and Python only; every result is an integer or a copied
row, so the GPU tests compare for equality."""
import numpy as np


def valid_faces(faces, n_vertices):
    """[F] bool: all three indices in [0, V)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < n_vertices)).all(1)


def components(faces, n_vertices):
    """(labels [V] int32, face_counts [V] int32, stats (components, components with a face, largest face count))"""
    V = int(n_vertices)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[valid_faces(f, V)]
    parent = list(range(V))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    # only the edges that can still join something: vectorised de-duplication, then the sequential union-find over what is left
    edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]]], 0)
    edges = edges[edges[:, 0] != edges[:, 1]]
    if edges.size:
        edges = np.unique(np.sort(edges, 1), axis=0)
    for a, b in edges.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)                      # the smaller id is the root: the root is the component's minimum
    labels = np.fromiter((find(v) for v in range(V)), np.int32, V)
    face_counts = np.zeros(V, np.int32)
    if f.shape[0]:
        np.add.at(face_counts, labels[f[:, 0]], 1)
    roots = labels == np.arange(V)
    stats = (int(roots.sum()), int((face_counts[roots] > 0).sum()), int(face_counts.max()) if V else 0)
    return labels, face_counts, stats


def filter_mesh(vertices, normals, colors, faces, threshold, labels=None, face_counts=None):
    """(vertices, normals, colors, faces, src, counts) of the components with face_count >= threshold: kept rows in their order, copied
    bit for bit; faces renumbered; normals / colors may be None"""
    V = int(np.asarray(vertices).shape[0])
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    if labels is None:
        labels, face_counts, _ = components(f, V)
    keep_v = face_counts[labels] >= threshold if V else np.zeros(0, bool)
    ok = valid_faces(f, V)
    keep_f = np.zeros(f.shape[0], bool)
    keep_f[ok] = keep_v[f[ok, 0]]
    src = np.flatnonzero(keep_v).astype(np.int32)
    new_id = np.full(V, -1, np.int32)
    new_id[src] = np.arange(src.size, dtype=np.int32)
    out_f = new_id[f[keep_f]].reshape(-1, 3)
    pick = lambda a: None if a is None else np.asarray(a)[src]      # noqa: E731
    return pick(vertices), pick(normals), pick(colors), out_f, src, (int(src.size), int(out_f.shape[0]))


def pieces(faces, n_vertices):
    """the faces of every component that has some, by label: {label: [n,3] faces}"""
    labels, _, _ = components(faces, n_vertices)
    f = np.asarray(faces).reshape(-1, 3)
    f = f[valid_faces(f, n_vertices)]
    of = labels[f[:, 0]]
    return {int(r): f[of == r] for r in np.unique(of)}
