"""Test infrastructure for the V-COCO role-AP evaluators (no GPU, no ctypes): a plain-loop restatement of the published
V-COCO toolkit's `_do_role_eval` (vsrl_eval.VCOCOeval; the toolkit is outside the reference tree, so this is the published
algorithm restated, parity unpinned at that boundary), and the seeded inputs the host and the GPU tests share.

`role_eval` reads the records of evaluate.vcoco_results the way the toolkit does (oracle.vsrl_consumer.
collect_detections_for_image: 26 actions x roles per record, template defaults for what a record does not carry), walks
every (action, role) of every image over the detections in descending score order with a `covered` flag per ground-truth
person, and scores each (action, role) with vsrl_consumer.voc_ap in float64.  Where the toolkit leaves the order of equal
scores to numpy's unstable argsort, the walk here is stable (earlier detection first)."""
import numpy as np
import torch

from oracle import vsrl_consumer as VC


def _overlap(boxes, ref):
    """The toolkit's get_overlap: IoU of every row of `boxes` with `ref`, pixel-index convention, in the arrays' fp32."""
    iw = np.maximum(np.minimum(boxes[:, 2], ref[2]) - np.maximum(boxes[:, 0], ref[0]) + np.float32(1), np.float32(0))
    ih = np.maximum(np.minimum(boxes[:, 3], ref[3]) - np.maximum(boxes[:, 1], ref[1]) + np.float32(1), np.float32(0))
    inters = iw * ih
    uni = ((ref[2] - ref[0] + np.float32(1)) * (ref[3] - ref[1] + np.float32(1)) +
           (boxes[:, 2] - boxes[:, 0] + np.float32(1)) * (boxes[:, 3] - boxes[:, 1] + np.float32(1)) - inters)
    return inters / uni


def role_eval(dets, vcocodb, scenario, template_rows=True, thr=0.5):
    """dets: the records of evaluate.vcoco_results; vcocodb: [{id, persons [G, 4], actions [G, 26], role_boxes [G, 26, 2, 4]}]
    (numpy); scenario 1 or 2.  template_rows=False keeps, of every record, only the (action, role) entry the record itself
    carries.  Returns (ap [26, 2] float64, NaN where undefined or no such role; own {image id: int8 [n records]} = the
    label each record got for its own entry, 1 / 0 / -1 (dropped); npos [26])."""
    nA = VC.NUM_ACTIONS
    tp = [[[] for _ in range(2)] for _ in range(nA)]
    sc = [[[] for _ in range(2)] for _ in range(nA)]
    npos = np.zeros(nA, np.int64)
    own = {}
    for entry in vcocodb:
        image_id = entry["id"]
        gt_boxes = np.asarray(entry["persons"], np.float32).reshape(-1, 4)
        gt_actions = np.asarray(entry["actions"]).reshape(-1, nA)
        gt_role_boxes = np.asarray(entry["role_boxes"], np.float32).reshape(-1, nA, 2, 4)
        ignore = np.any(gt_actions == -1, axis=1)
        npos += np.sum(gt_actions == 1, axis=0)
        mine = [d for d in dets if d["image_id"] == image_id]
        pred_agents, pred_roles = VC.collect_detections_for_image(dets, image_id)
        own[image_id] = np.zeros(len(mine), np.int8)
        for aid, (action, roles) in enumerate(VC.ACTION_ROLES):
            for rid in range(len(roles) - 1):
                covered = np.zeros(gt_boxes.shape[0], bool)
                gt_roles = gt_role_boxes[:, aid, rid]
                is_own = np.array([(action + "_" + roles[rid + 1]) in d for d in mine], bool)
                agent_scores = pred_roles[:, 5 * aid + 4, rid]
                for j in np.argsort(-agent_scores, kind="stable"):       # NaN scores sort last and are skipped
                    if not (template_rows or is_own[j]):
                        continue
                    if np.isnan(agent_scores[j]):
                        if is_own[j]:
                            own[image_id][j] = -1
                        continue
                    hit = False
                    if gt_boxes.shape[0]:                                # (the toolkit's images always hold a person)
                        overlaps = _overlap(gt_boxes, pred_agents[j, :4])
                        jmax = int(overlaps.argmax()); ovmax = overlaps.max()
                        if ignore[jmax]:
                            if is_own[j]:
                                own[image_id][j] = -1
                            continue
                        role_box = pred_roles[j, 5 * aid:5 * aid + 4, rid]
                        if np.all(gt_roles[jmax] == -1):
                            if scenario == 1:
                                ov_role = 1.0 if (np.all(role_box == 0.0) or np.all(np.isnan(role_box))) else 0.0
                            else:
                                ov_role = 1.0
                        else:
                            ov_role = _overlap(gt_roles[jmax].reshape(1, 4), role_box)[0]
                        if gt_actions[jmax, aid] == 1 and ovmax >= thr and ov_role >= thr and not covered[jmax]:
                            covered[jmax] = True
                            hit = True
                    sc[aid][rid].append(float(agent_scores[j])); tp[aid][rid].append(1.0 if hit else 0.0)
                    if is_own[j]:
                        own[image_id][j] = 1 if hit else 0
    ap = np.full((nA, 2), np.nan)
    for aid, (_, roles) in enumerate(VC.ACTION_ROLES):
        for rid in range(len(roles) - 1):
            if npos[aid] == 0:
                continue
            a_sc = np.asarray(sc[aid][rid], np.float64); a_tp = np.asarray(tp[aid][rid], np.float64)
            order = np.argsort(-a_sc, kind="stable")
            c_tp = np.cumsum(a_tp[order]); c_fp = np.cumsum(1.0 - a_tp[order])
            ap[aid, rid] = VC.voc_ap(c_tp / float(npos[aid]), c_tp / np.maximum(c_tp + c_fp, np.finfo(np.float64).eps))
    return ap, own, npos


def all_point_ap(labels_sorted, num_gt):
    """VOC all-point AP of one class's labels in score order through vsrl_consumer.voc_ap (float64); 0 without ground truth
    or detections, like the device kernels."""
    lab = np.asarray(labels_sorted, np.float64)
    if num_gt <= 0 or lab.size == 0:
        return 0.0
    tp = np.cumsum(lab); fp = np.cumsum(1.0 - lab)
    return VC.voc_ap(tp / float(num_gt), tp / np.maximum(tp + fp, np.finfo(np.float64).eps))


def _int_boxes(rs, n):
    xy = rs.randint(0, 300, (n, 2)); wh = rs.randint(20, 200, (n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def make_case(seed, actions, n_images=6, big_image=None):
    """Seeded head outputs and V-COCO targets in integer pixel coordinates (every area, intersection and threshold
    comparison is exact in fp32).  Pairs share a few human and object boxes, so that cells of one class contest a person;
    scores have one decimal in (0, 1] (many ties); ground-truth persons are integer-jittered copies of detected human
    boxes, some duplicated exactly, with role boxes jittered from the detected ones (never smaller than 2 x 2) or absent
    (-1).  Image 0 carries a detected role box of all zeros under a role-less ground truth and a NaN score; image 2 an
    ignored person on top of a detected box; image 3 has no detections; image 4 no persons; image 5 five persons of which
    two are the same box.  big_image: that image gets 40 pairs x 7 or 8 classes (280 cells at least).
    Returns (outputs, targets, image_ids, class table [(aid, rid)])."""
    rs = np.random.RandomState(seed)
    names = [a for a, _ in VC.ACTION_ROLES]
    table = []
    for a in actions:
        act, role = a.split()
        table.append((names.index(act), VC.ACTION_ROLES[names.index(act)][1].index(role) - 1))
    K = len(actions)
    outs, tgts = [], []
    for b in range(n_images):
        n_pairs = 0 if b == 3 else (40 if b == big_image else rs.randint(4, 10))
        humans = _int_boxes(rs, max(1, n_pairs // 3)); objects = _int_boxes(rs, n_pairs // 2 + 1)
        bh = humans[rs.randint(0, len(humans), n_pairs)].reshape(-1, 4)
        bo = objects[rs.randint(0, len(objects), n_pairs)].reshape(-1, 4)
        if b == 0:
            bo[0] = 0.0                                                   # "no role object predicted"
        index, pred = [], []
        for p in range(n_pairs):
            for k in rs.choice(K, size=rs.randint(7, 9) if b == big_image else rs.randint(1, 5), replace=False):
                index.append(p); pred.append(int(k))
        index = np.asarray(index, np.int64); pred = np.asarray(pred, np.int64)
        scores = np.round(rs.uniform(0.06, 1.0, len(index)), 1).astype(np.float32)
        if b == 0:
            scores[len(scores) // 2] = np.nan
        persons, acts, roles = [], [], []

        def person(box, cells, roleless=False, ignored=False, twice=False):
            a = np.zeros(26, np.int64); r = np.full((26, 2, 4), -1.0, np.float32)
            for c in cells:
                aid, rid = table[int(pred[c])]
                a[aid] = 1
                if not roleless and bo[index[c]].any():
                    r[aid, rid] = bo[index[c]] + rs.randint(-4, 5, 4)
            if ignored:
                a[rs.randint(0, 26, 3)] = -1
            for _ in range(2 if twice else 1):
                persons.append(box.copy()); acts.append(a.copy()); roles.append(r.copy())

        if b == 4 or n_pairs == 0:
            chosen = []
        else:
            chosen = list(rs.permutation(len(index))[:4 if b == 5 else rs.randint(2, 6)])
        for i, c in enumerate(chosen):
            p = index[c]
            cells = [c] + [d for d in np.nonzero(index == p)[0] if d != c and rs.uniform() < 0.5][:1]
            person(bh[p] + rs.randint(-4, 5, 4), cells, roleless=rs.uniform() < 0.3,
                   twice=(i == 0) if b == 5 else rs.uniform() < 0.25)
        if b == 0:                                                        # the role-less person behind the empty role box
            person(bh[0] + rs.randint(-2, 3, 4), list(np.nonzero(index == 0)[0]), roleless=True)
        if b == 2:
            person(bh[index[0]].copy(), [0], ignored=True)
        if b not in (4, 5) and rs.uniform() < 0.5:                        # a person nobody detected
            a = np.zeros(26, np.int64); a[rs.randint(0, 26)] = 1
            persons.append(_int_boxes(rs, 1)[0]); acts.append(a); roles.append(np.full((26, 2, 4), -1.0, np.float32))
        G = len(persons)
        tgts.append(dict(persons=torch.tensor(np.asarray(persons, np.float32).reshape(G, 4)),
                         actions=torch.tensor(np.asarray(acts, np.int64).reshape(G, 26)),
                         role_boxes=torch.tensor(np.asarray(roles, np.float32).reshape(G, 26, 2, 4))))
        outs.append(dict(boxes_h=torch.tensor(bh), boxes_o=torch.tensor(bo), index=torch.tensor(index),
                         prediction=torch.tensor(pred), scores=torch.tensor(scores)))
    return outs, tgts, [100 + b for b in range(n_images)], table


def vcocodb_of(targets, image_ids):
    return [dict(id=i, persons=t["persons"].numpy(), actions=t["actions"].numpy(), role_boxes=t["role_boxes"].numpy())
            for t, i in zip(targets, image_ids)]
