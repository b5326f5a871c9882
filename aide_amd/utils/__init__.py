# mirrors the reference's utils/__init__.py:1-10 for the hot-path symbols
from .loss2d import (CrossEntropyLoss2d, DiceLoss, CEDiceLoss, CEMDiceLoss, MulticlassDiceLoss, Dice_Loss,  # noqa: F401
                     MulticlassMSELoss, CEMDiceLossImage)
from .metrics2d import (Dice_fn, IoU_fn, TP_TN_FP_FN, MulticlassDice_fn, MulticlassIoU_fn, MulticlassTP_TN_FP_FN,  # noqa: F401
                        MulticlassAccuracy_fn, Dice_fn_Nozero, one_hot_result, multiclass_counts, MulticlassMeter)
from .coteach_loss import (Coteachingloss_dropimage, Coteachingloss_weightimage, Coteachingloss_dropregionce,  # noqa: F401
                           Coteachingloss_dropimagedroppixel, KLbidirection, CoTeachingProposedLoss,
                           pseudo_label_ensemble)
from .augment import reverseaug, reverse_aug_tensor  # noqa: F401
from .loader_aug import LoaderAugment, draw_aug_params, CHAOS_PALETTE  # noqa: F401
from .reg_loss import Pixelcoreg_Focalloss, Pixelcoreg_Focalloss_twomodel  # noqa: F401
from .poly_lr_scheduler import PolyLR  # noqa: F401
from .metrics3d import surface_scores, RAVD3d_fn, ASSD3d_fn, MSSD3d_fn, HD95_fn, NSD3d_fn  # noqa: F401
