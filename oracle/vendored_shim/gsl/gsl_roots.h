/* Empty on purpose: nothing of this header is used on the path polar_ref builds. */
#pragma once
