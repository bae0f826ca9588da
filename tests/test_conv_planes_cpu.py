"""Host side of the conv-tap addressing: the row map of hip.x3_conv_row - the Python twin of the kernels' x3_conv_row - against an index image
padded by torch, and the tap shifts in that row space."""
import torch
import torch.nn.functional as F


def test_row_map_and_tap_shifts_address_the_zero_bordered_image():
    import pixelspointspolygons_amd.hip as hip
    B, H, W = 3, 5, 7
    idx = torch.arange(1, B * H * W + 1, dtype=torch.float32).view(B, 1, H, W)                # pixel m holds m + 1; the border holds 0
    img = F.pad(idx, (1, 1, 1, 1)).view(-1)
    Pw = W + 2
    rows = [hip.x3_conv_row(m, H, W) for m in range(B * H * W)]
    assert [int(img[r]) for r in rows] == list(range(1, B * H * W + 1))
    assert len(set(rows)) == len(rows) and min(rows) == Pw + 1 and max(rows) == B * (H + 2) * Pw - Pw - 2
    # every tap of every interior pixel stays inside the pixel's own padded image and reads what a 3 x 3 window over the padded image reads
    win = F.unfold(F.pad(idx, (1, 1, 1, 1)), 3).view(B, 9, H * W)                            # [b, tap, pixel]
    for m, r in enumerate(rows):
        b, p = divmod(m, H * W)
        for t in range(9):
            s = (t // 3 - 1) * Pw + (t % 3 - 1)
            assert b * (H + 2) * Pw <= r + s < (b + 1) * (H + 2) * Pw
            assert float(img[r + s]) == float(win[b, t, p])
