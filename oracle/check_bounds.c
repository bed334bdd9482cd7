/* check_bounds.c — TEST INFRASTRUCTURE ONLY: `make check-bounds` compiles this with
 * chess_oracle.c under -fsanitize=address,undefined and runs it.  It calls every function
 * that keeps a move list on boards with more legal moves than ZCC_MAX_MOVES (no game reaches
 * them): a write past a buffer ends the run with the sanitizer's report. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "c4_oracle.h"
#include "chess_oracle.h"

static int failures;

#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "check_bounds:%d: %s\n", __LINE__, #cond);    \
            failures++;                                                   \
        }                                                                 \
    } while (0)

static void set_board(zcc_state *s, const char *board, int turn) {
    memset(s, 0, sizeof *s);
    memcpy(s->board, board, 64);
    s->turn = (uint8_t)turn;
}

static void light_of(const zcc_state *s, zcc_light *l) {
    memcpy(l->board, s->board, 64);
    l->turn = s->turn;
    l->fifty = s->fifty;
    l->castle = s->castle;
    l->pad = 0;
}

/* The list functions on one over-capacity board; `want` > 0: the exact count. */
static void over_capacity(const char *name, const char *board, int want) {
    zcc_state *s = (zcc_state *)malloc(sizeof *s);
    /* exactly ZCC_MAX_MOVES entries on the heap: the sanitizer sees entry 256 */
    zcc_move *out = (zcc_move *)malloc(sizeof(zcc_move) * ZCC_MAX_MOVES);
    set_board(s, board, 0);
    const int n = zcc_legal_moves(s, out);
    printf("%s: %d legal moves\n", name, n);
    EXPECT(n > ZCC_MAX_MOVES);
    if (want > 0) EXPECT(n == want);
    EXPECT(zcc_check_win(s) == 0);
    EXPECT(zcc_check_draw(s) == 0);
    EXPECT(zcc_perft(s, 1) == (uint64_t)n);
    EXPECT(zcc_perft(s, 2) == UINT64_MAX);
    zcc_light l;
    light_of(s, &l);
    (void)zcc_crude_score(&l);
    zco_mt *mt = (zco_mt *)calloc(1, sizeof *mt);
    zco_mt_seed(mt, 5);
    int *na = (int *)malloc(sizeof(int) * ZCC_MAX_MOVES), n_root = -1;
    for (int policy = 0; policy < 2; policy++)
        EXPECT(zcc_get_move(&l, mt, 40, 1.4, 8, policy, 3.0, NULL, NULL, na, out, &n_root) == -2);
    EXPECT(n_root == ZCC_MAX_MOVES);
    int plies = -1;
    EXPECT(zcc_rollout(s, mt, &plies) == 3);
    EXPECT(plies == 0);
    uint64_t exp = 0;
    EXPECT(zcc_selfplay_batch(1, &l, mt, 2, 20, 1.4, 8, 1, 3.0, 1, &exp) == 0);
    free(na);
    free(mt);
    free(out);
    free(s);
}

int main(void) {
    /* 277 pseudo-legal and legal moves: a ring of queens round an empty centre */
    over_capacity("queen ring", "KQQQQQQQQ      QQ      QQ      QQ      QQ      QQ      QQQQQQQQk", 277);
    char q62[65];
    memset(q62, 'Q', 64);
    q62[64] = 0;
    q62[0] = 'K';
    q62[63] = 'k';
    /* 62 queens: no empty square, every move a capture - none exists (the king is never taken) */
    zcc_state *s = (zcc_state *)malloc(sizeof *s);
    zcc_move *out = (zcc_move *)malloc(sizeof(zcc_move) * ZCC_MAX_MOVES);
    set_board(s, q62, 0);
    printf("62 queens: %d legal moves\n", zcc_legal_moves(s, out));
    /* 62 queens of the side to move round ten empty squares and the kings in the corners:
     * the widest scratch use this file tries */
    memcpy(q62, "KQQQQQQQQ QQ QQQQQQQQQQQQQ QQ QQQQ QQ QQQQQQQQQQQQQ QQ QQQQQQQQk", 64);
    set_board(s, q62, 0);
    printf("queens and holes: %d legal moves\n", zcc_legal_moves(s, out));
    /* bytes that are no piece at all */
    memset(s->board, 0xFF, 64);
    (void)zcc_legal_moves(s, out);
    memset(s->board, 0, 64);
    (void)zcc_legal_moves(s, out);
    free(out);
    free(s);
    if (failures) return 1;
    printf("check-bounds ok\n");
    return 0;
}
