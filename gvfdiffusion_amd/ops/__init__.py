"""Operator-level Python bindings; importing this package registers every C-ABI signature."""
from .. import _lib  # noqa: F401
from . import dit_ops  # noqa: F401
from . import vae_ops  # noqa: F401
from . import image_loss  # noqa: F401
from . import knn_interp  # noqa: F401
from . import attention_grad  # noqa: F401
from . import optim  # noqa: F401
from . import dit_train  # noqa: F401
from . import linear_grad  # noqa: F401
from . import lpips  # noqa: F401
from . import sparse_train  # noqa: F401
from . import vae_train  # noqa: F401
from . import spconv  # noqa: F401
from . import conv3d  # noqa: F401
from . import vit  # noqa: F401
from . import clip  # noqa: F401
from ..sparse import vox2seq as _vox2seq  # noqa: F401,E402
