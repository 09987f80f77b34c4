"""Shared body of the pile-harvest-on-reset tests of BlockAssemblyOrient (OR:1463-1488) and BlockAssemblySearch (SE:1289-1343,
1367-1421): tests/test_gpu_orient_parity.py / tests/test_gpu_search_parity.py on the GPU, tests/test_hipemu_task_parity.py on the
emulator.  One simulator step, then a masked reset_idx with the accept rule's inputs set by hand."""
import numpy as np
import torch

SEARCH_PIXEL_THRESHOLD = np.array([20, 20, 15, 20, 20, 30, 30, 20], np.float32)      # by brick-type group, SE:1289


def check_pile_harvest_on_reset(task_kind, scene, **desc_overrides):
    import seqdex_amd.sim as S            # (looked up at call time: the emulator suite substitutes the simulator class)
    assert task_kind in (1, 3)
    n = 16
    s = S.SdxSim(n, device="cuda:0", seed=7, task_kind=task_kind, **desc_overrides)
    try:
        env = np.arange(n)
        seg = np.array([scene.seg_index(e) for e in range(n)])
        pile0 = s.ROOT.view(n, 142, 13)[0, 9:141].cpu().numpy().copy()              # the default saved pile (K = 1): the spawn lattice
        s.RESET.zero_()
        s.step(torch.zeros(n, 23).cuda())                                           # total_steps = 1, no reset event
        torch.cuda.synchronize()
        reject = env % 3 == 0
        masked = env % 4 != 1
        root = s.ROOT.view(n, 142, 13)
        if task_kind == 1:
            fd = np.where(reject, 0.2, 0.4).astype(np.float32)
            s.FINGER_DIST.copy_(torch.from_numpy(fd).cuda())
            s.TVALUE.fill_(1.0)
            for e in range(n):
                root[e, int(seg[e]), 1] = 0.25
            torch.cuda.synchronize()
            y = s.ROOT.view(n, 142, 13).cpu().numpy()[env, seg, 1]
            good = (fd > 0.3) & (y > 0.0) & (y < 0.5) & (s.TVALUE.cpu().numpy() > 0.6)           # OR:1468-1470
        else:
            pix = torch.zeros(n, 4)
            pix[:, 0] = torch.from_numpy(SEARCH_PIXEL_THRESHOLD[env % 8] + np.where(reject, 0.0, 1.0).astype(np.float32))
            s.SEG_PIXELS.copy_(pix.cuda())
            good = pix[:, 0].numpy() > SEARCH_PIXEL_THRESHOLD[env % 8]                           # SE:1289
        np.testing.assert_array_equal(good, ~reject)
        torch.cuda.synchronize()
        root_before = s.ROOT.view(n, 142, 13).cpu().numpy().copy()
        cam_before = s.CAM_ROT.cpu().numpy().copy()
        s.reset_idx(torch.from_numpy(masked.astype(np.uint8)).cuda())
        torch.cuda.synchronize()

        acc = good & masked
        want_count = np.bincount(env[acc] % 8, minlength=8)
        np.testing.assert_array_equal(want_count, [1, 0, 2, 1, 1, 0, 1, 1])
        np.testing.assert_array_equal(s.PILE_HARVEST_COUNT.cpu().numpy(), want_count)
        np.testing.assert_array_equal(s.TV_COUNT.cpu().numpy(), [7, 5])
        assert int(acc.sum()) == 7 and int((masked & ~good).sum()) == 5
        ring = s.PILE_HARVEST.cpu().numpy()
        keys = s.PILE_HARVEST_KEYS.cpu().numpy()
        for grp in range(8):
            k = int(want_count[grp])
            want_keys = sorted((1 << 24) | int(e) for e in env[acc & (env % 8 == grp)])
            assert sorted(int(v) for v in keys[grp, :k]) == want_keys, grp                       # in any slot order
            for slot in range(k):
                e = int(keys[grp, slot]) & 0xFFFFFF
                assert ring[grp, slot].shape == (132, 13)
                np.testing.assert_array_equal(ring[grp, slot].view(np.uint32), root_before[e, 9:141].view(np.uint32))
        tvk = s.TV_KEYS
        succ = s.ring_rows(s.TV_SUCCESS, tvk[0], 7).cpu().numpy()
        fail = s.ring_rows(s.TV_FAILURE, tvk[1], 5).cpu().numpy()
        np.testing.assert_array_equal(succ.view(np.uint32), cam_before[acc].view(np.uint32))
        np.testing.assert_array_equal(fail.view(np.uint32), cam_before[masked & ~good].view(np.uint32))
        if task_kind == 3:
            np.testing.assert_array_equal(s.SUCCESS_BUF.cpu().numpy()[masked], good[masked].astype(np.int64))
        root_after = s.ROOT.view(n, 142, 13).cpu().numpy()
        np.testing.assert_array_equal(root_after[~masked].view(np.uint32), root_before[~masked].view(np.uint32))
        assert not s.PROGRESS.cpu().numpy()[masked].any() and not s.RESET.cpu().numpy()[masked].any()
        if task_kind == 3:
            d = s._desc
            pose = np.array(list(d.search_default_arm) + list(d.search_finger_pose), np.float32)
            dof = s.DOF.view(n, 23, 2).cpu().numpy()
            tg, ptg = s.TARGETS.cpu().numpy(), s.PREV_TARGETS.cpu().numpy()
            for e in env[masked]:
                t = root_after[e, seg[e]].astype(np.float64)
                assert t[2] == np.float64(np.float32(0.9))
                r = (t[0] - 0.25) / 0.2
                assert abs(r - (t[1] - 0.19) / 0.15) <= 1e-5 and -1.0 <= r <= 1.0, (e, t[:3])
                others = np.ones(132, bool)
                others[seg[e] - 9] = False
                free = others.copy()
                free[72:] = False
                b = root_after[e, 9:141]
                assert np.abs(b[free, 0:2].astype(np.float64) - pile0[free, 0:2].astype(np.float64)).max() <= 0.02, e
                np.testing.assert_array_equal(b[free, 2:7], pile0[free, 2:7])
                np.testing.assert_array_equal(b[others & ~free, 0:7], pile0[others & ~free, 0:7])
                assert not b[others, 7:13].any()
                np.testing.assert_array_equal(dof[e, :, 0], pose)
                assert not dof[e, :, 1].any()
                np.testing.assert_array_equal(tg[e], pose)
                np.testing.assert_array_equal(ptg[e], pose)
    finally:
        s.close()
