"""COLMAP 3.11's CorrespondenceGraph as COLMAP states it, in plain Python: the restatement mpsfm_corr_graph_build is tested against.

AddCorrespondences (scene/correspondence_graph.cc): a list between an image and itself is refused whole; a match with an index
outside an image's keypoints is refused; a match whose partner already stands in the keypoint's list is a duplicate and refused;
every other match is appended to the lists of both keypoints.  Finalize: the lists are put in order (COLMAP leaves them in arrival
order; the library's contract is ascending global keypoint index, which is what the track engine's arrays have always had) and the
per-image counts are taken.  Lists arrive in the order of the input, matches in the order of a list, so "already stands in the list"
is "occurs at a lower position".

Nothing here is shared with mpsfm_amd: per-keypoint Python lists, a linear duplicate search, sorted() at the end."""

import numpy as np

ADDED, INVALID, SELF_PAIR, DUPLICATE = 0, 1, 2, 3


def build(kp_start, list_image0, list_image1, list_start, matches):
    """The outputs of mpsfm_corr_graph_build, under the names of capi.corr_graph_build (no `info`)."""
    kp_start = [int(v) for v in kp_start]
    n_images = len(kp_start) - 1
    nkp = [kp_start[i + 1] - kp_start[i] for i in range(n_images)]
    corrs = [[[] for _ in range(n)] for n in nkp]  # corrs[image][point2D] = [(image, point2D)]
    matches = np.asarray(matches, np.int64).reshape(-1, 2)
    status = np.zeros(len(matches), np.uint8)
    for l, (a, b) in enumerate(zip(list_image0, list_image1)):
        a, b = int(a), int(b)
        for m in range(int(list_start[l]), int(list_start[l + 1])):
            i0, i1 = int(matches[m, 0]), int(matches[m, 1])
            if a == b:
                status[m] = SELF_PAIR
            elif not (0 <= i0 < nkp[a] and 0 <= i1 < nkp[b]):
                status[m] = INVALID
            elif any(c == (b, i1) for c in corrs[a][i0]):
                status[m] = DUPLICATE
            else:
                corrs[a][i0].append((b, i1))
                corrs[b][i1].append((a, i0))
    # Finalize
    corr_start, corr_kp, two_view = [0], [], []
    num_corr, num_obs = np.zeros(n_images, np.int32), np.zeros(n_images, np.int32)
    pairs = {}
    for a in range(n_images):
        for i0 in range(nkp[a]):
            row = sorted(kp_start[b] + i1 for b, i1 in corrs[a][i0])
            corr_kp += row
            corr_start.append(len(corr_kp))
            num_corr[a] += len(row)
            num_obs[a] += 1 if row else 0
            two_view.append(1 if len(row) == 1 and len(corrs[corrs[a][i0][0][0]][corrs[a][i0][0][1]]) == 1 else 0)
            for b, i1 in corrs[a][i0]:
                if a < b:
                    pairs.setdefault((a, b), []).append((i0, i1))
    keys = sorted(pairs)
    pair_matches = [m for k in keys for m in sorted(pairs[k])]
    pair_start = np.concatenate([[0], np.cumsum([len(pairs[k]) for k in keys])]).astype(np.int64)
    return dict(match_status=status, corr_start=np.array(corr_start, np.int64), corr_kp=np.array(corr_kp, np.int64),
                image_num_correspondences=num_corr, image_num_observations=num_obs, kp_two_view=np.array(two_view, np.uint8),
                pair_image0=np.array([k[0] for k in keys], np.int32), pair_image1=np.array([k[1] for k in keys], np.int32),
                pair_start=pair_start, pair_matches=np.array(pair_matches, np.int32).reshape(-1, 2))


OUTPUTS = ("match_status", "corr_start", "corr_kp", "image_num_correspondences", "image_num_observations", "kp_two_view", "pair_image0",
           "pair_image1", "pair_start", "pair_matches")


def assert_equal(got, want, skip=()):
    """every output: the same dtype, shape and values"""
    for name in OUTPUTS:
        if name in skip:
            continue
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (name, np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))[:10])


def lists_of(groups):
    """[(image0, image1, [[i0, i1], ...])] -> list_image0, list_image1, list_start, matches"""
    li0 = np.array([g[0] for g in groups], np.int32)
    li1 = np.array([g[1] for g in groups], np.int32)
    ms = [np.asarray(g[2], np.int32).reshape(-1, 2) for g in groups]
    start = np.concatenate([[0], np.cumsum([len(m) for m in ms])]).astype(np.int64)
    return li0, li1, start, (np.concatenate(ms) if ms else np.zeros((0, 2), np.int32))
